"""Plain NumPy restatements of the dense-array hooks whose result is a layout rule and no arithmetic worth the name (include/hpgmg_operators.h
hpgmg_dense_pack / _pack_walls / _unpack, hpgmg_boundary_restrict / _store_walls / _check_kappa), for tests/test_oracle_dense_hooks.py (which pins
each on the CPU oracle, bit for bit) and tests/test_gpu_dense_hooks.py (which holds the HIP kernels to them).  Nothing here reads the code under
test: a level enters as its geometry (Geo), a vector as its padded boxes, an array of shape (boxes, volume) as hpgmg_testlib.Level.read_all gives it.

A padded box holds cell (i, j, k), i fastest, -ghosts <= i, j, k < dim + ghosts, at (i + ghosts) + (j + ghosts) * jStride + (k + ghosts) * kStride;
the strides pad a row and a plane, and the volume pads the box.  Dense arrays are [k][j][i]; a boundary array is (6, n, n): faces 0, 1 (i-low,
i-high) indexed [k][j], 2, 3 (j) indexed [k][i], 4, 5 (k) indexed [j][i].
"""
import numpy as np

import hpgmg_amd as H

# (boxes per side, box side) of the single-level tests.  (1, 162): jStride 164, kStride 26896, a padded volume of 4,410,944 doubles and 4,251,528
# cells, both above the 16384 workgroups x 256 lanes = 4,194,304 of one grid-stride trip of kernels/dense_io.hip, dense_boundary.hip and
# dense_flux.hip; 161^3 = 4,173,281 is below.  (3, 12): a middle box on no wall, boxes on one, two and three walls.  (17, 2): 4913 boxes.
GEOMS = [(1, 162), (3, 12), (17, 2), (1, 6), (1, 1)]
TRIP = 16384 * 256
MIXED = 0b011010                                      # i-high, j-high and k-low are masked walls; the other three Dirichlet
WALLS = [("dirichlet", 0, False), ("neumann", 63, False), ("mixed-kappa", MIXED, True)]      # (name, mask, with a kappa array)
VECTORS = 10                                          # TEMP .. ALPHA: the vectors the hooks and these tests name
LAYOUTS = [H.DENSE_CELL, H.DENSE_FACE_I, H.DENSE_FACE_J, H.DENSE_FACE_K]


def wall_masks(axis):
    """For pack_walls of a face array of `axis`: mask 0, all six, the mixed one, only the low and only the high wall of that axis."""
    return [0, 63, MIXED, 1 << (2 * axis), 1 << (2 * axis + 1)]


# hpgmg_boundary_check_kappa: (name, [(face, q, p, value)] planted into an all-zero array, robin_mask, status, any_positive); q, p < 0 count from the end
KAPPA_CASES = [
    ("clean", [], 63, 0, 0),
    ("nan on a face that is not Robin", [(0, 0, 0, np.nan)], 0b111110, H.DENSE_NOT_FINITE, 0),
    ("inf in the last entry", [(5, -1, -1, np.inf)], 0, H.DENSE_NOT_FINITE, 0),
    ("negative on a face that is not Robin", [(2, -1, 0, -1.0)], 0b111011, 0, 0),
    ("negative on a Robin face", [(2, -1, 0, -1.0)], 0b000100, H.DENSE_OUT_OF_RANGE, 0),
    ("positive in the last entry of face 5, Robin", [(5, -1, -1, 0.25)], 0b100000, 0, 1),
    ("positive in the last entry of face 5, not Robin", [(5, -1, -1, 0.25)], 0b011111, 0, 0),
    ("minus zero on a Robin face", [(1, 0, -1, -0.0)], 63, 0, 0),
    ("nan and negative", [(0, 0, 0, np.nan), (3, 0, -1, -2.0)], 0b001000, H.DENSE_NOT_FINITE | H.DENSE_OUT_OF_RANGE, 0),
]


def kappa_case(n, plants):
    kappa = np.zeros((6, n, n))
    for face, q, p, value in plants:
        kappa[face, q, p] = value
    return kappa


def geom_id(v):
    return f"{v[0]}x{v[1]}" if isinstance(v[0], int) else v[0]          # a geometry, or the name of a WALLS entry


class Geo:
    """What a restatement may know of a level: sizes, strides and where each box sits."""

    def __init__(self, level, periodic=False):
        self.n, self.dim, self.g = level.dim, level.box_dim, level.ghosts
        self.jS, self.kS, self.vol, self.boxes = level.jStride, level.kStride, level.volume, level.num_boxes
        self.lows = [level.box_low(b) for b in range(level.num_boxes)]          # (i, j, k) of the first cell of each box
        self.periodic = periodic

    def offsets(self, ei, ej, ek):
        """Padded offsets of the local cells [0, ek) x [0, ej) x [0, ei), as a (ek, ej, ei) array."""
        g = self.g
        return ((np.arange(ek) + g) * self.kS)[:, None, None] + ((np.arange(ej) + g) * self.jS)[None, :, None] + (np.arange(ei) + g)[None, None, :]

    def extents(self, low, layout):
        """Cells per axis (i, j, k) of a box that a dense array of `layout` determines: dim, and one more along the array's axis when the box
        lies on the domain's high face of it and the domain is not periodic (the high ghost layer)."""
        e = [self.dim] * 3
        axis = layout - H.DENSE_FACE_I
        if axis >= 0 and not self.periodic and low[axis] + self.dim == self.n:
            e[axis] += 1
        return e


def dense_shape(geo, layout):
    s = [geo.n] * 3                                  # (k, j, i)
    if layout != H.DENSE_CELL and not geo.periodic:
        s[2 - (layout - H.DENSE_FACE_I)] += 1
    return tuple(s)


def pack(geo, src, layout):
    """The padded boxes after hpgmg_dense_pack: zeros everywhere, then what the array determines."""
    out = np.zeros((geo.boxes, geo.vol))
    for b, low in enumerate(geo.lows):
        ei, ej, ek = geo.extents(low, layout)
        out[b][geo.offsets(ei, ej, ek)] = src[low[2]:low[2] + ek, low[1]:low[1] + ej, low[0]:low[0] + ei]
    return out


def unpack(geo, boxes, layout=H.DENSE_CELL):
    """The gather that undoes pack; CELL: hpgmg_dense_unpack (interior cells only).  Entries no box determines stay NaN: there are none."""
    out = np.full(dense_shape(geo, layout), np.nan)
    for b, low in enumerate(geo.lows):
        ei, ej, ek = geo.extents(low, layout)
        out[low[2]:low[2] + ek, low[1]:low[1] + ej, low[0]:low[0] + ei] = boxes[b][geo.offsets(ei, ej, ek)]
    return out


def pack_walls(geo, src, layout, mask, wall):
    """(padded boxes, wall array) after hpgmg_dense_pack_walls on a Dirichlet cube: a masked wall of the array's axis (entries 0 / n along it) moves
    to face 2 axis / 2 axis + 1 of `wall` and leaves 0.0 in the vector; every other entry of `wall` keeps what it held."""
    axis = layout - H.DENSE_FACE_I
    src, wall = src.copy(), wall.copy()
    for side, at in ((0, 0), (1, geo.n)):
        if (mask >> (2 * axis + side)) & 1:
            where = [slice(None)] * 3
            where[2 - axis] = at
            wall[2 * axis + side] = src[tuple(where)]          # [k][j], [k][i], [j][i]: the two remaining axes in their order
            src[tuple(where)] = 0.0
    return pack(geo, src, layout), wall


def restrict(g_f):
    """hpgmg_boundary_restrict: the four finer entries under each entry, summed left to right, times 0.25."""
    return (g_f[:, 0::2, 0::2] + g_f[:, 0::2, 1::2] + g_f[:, 1::2, 0::2] + g_f[:, 1::2, 1::2]) * 0.25


def store_walls(geo, betas, wall, kappa, h, mask):
    """The three beta vectors (padded boxes) after hpgmg_boundary_store_walls: on a masked wall the face's beta -- index 0 along the axis in a box
    on the low wall, the high ghost layer dim in a box on the high wall -- becomes wall * (t / (2.0 + t)), t = kappa * h (kappa None: t = 0.0);
    nothing else changes."""
    out = [b.copy() for b in betas]
    d, g = geo.dim, geo.g
    stride = (1, geo.jS, geo.kS)
    for face in range(6):
        if not (mask >> face) & 1:
            continue
        axis, high = face >> 1, face & 1
        pa, qa = [a for a in range(3) if a != axis]                                  # the face's faster and slower axis: (j, k), (i, k), (i, j)
        t = (kappa[face] if kappa is not None else np.zeros((geo.n, geo.n))) * h
        value = wall[face] * (t / (2.0 + t))
        for b, low in enumerate(geo.lows):
            if low[axis] != (geo.n - d if high else 0):
                continue
            at = (g + (d if high else 0)) * stride[axis]
            offs = at + ((np.arange(d) + g) * stride[qa])[:, None] + ((np.arange(d) + g) * stride[pa])[None, :]
            out[axis][b][offs] = value[low[qa]:low[qa] + d, low[pa]:low[pa] + d]
    return out


def check_kappa(kappa, robin_mask):
    """(status, any_positive) of hpgmg_boundary_check_kappa: NOT_FINITE for a value that is not finite anywhere; on the faces of robin_mask
    OUT_OF_RANGE for a negative one and any_positive for one above zero."""
    status, positive = 0, 0
    if not np.isfinite(kappa).all():
        status |= H.DENSE_NOT_FINITE
    for face in range(6):
        if (robin_mask >> face) & 1:
            v = kappa[face][np.isfinite(kappa[face])]
            if (v < 0.0).any():
                status |= H.DENSE_OUT_OF_RANGE
            if (v > 0.0).any():
                positive = 1
    return status, positive


def check_bits(a, check):
    """The status of a pack of the values a: NOT_FINITE, and OUT_OF_RANGE for a finite value that fails `check`."""
    finite = np.isfinite(a)
    v = a[finite]
    bad = (check == H.DENSE_CHECK_POSITIVE and not (v > 0.0).all()) or (check == H.DENSE_CHECK_NONNEGATIVE and not (v >= 0.0).all())
    return (0 if finite.all() else H.DENSE_NOT_FINITE) | (H.DENSE_OUT_OF_RANGE if bad else 0)


def _patterns(a, computed_nan):
    a = np.ascontiguousarray(a)
    if computed_nan:
        a = np.where(np.isnan(a), np.nan, a)
    return a.view(np.uint64)


def same_bits(a, b, computed_nan=False):
    """Whether two arrays hold the same 64-bit patterns: the sign of a zero counts, and so do the sign and payload of a NaN -- unless
    computed_nan: a NaN then equals any NaN in the same place.  That is for the result of arithmetic on a planted NaN, whose sign and payload
    IEEE 754 leaves open (a compiler may turn a - b into a + (-b)); a NaN that is only copied keeps its bits and is compared with them."""
    return np.shape(a) == np.shape(b) and np.array_equal(_patterns(a, computed_nan), _patterns(b, computed_nan))


def first_differences(a, b, limit=5, computed_nan=False):
    bad = np.argwhere(_patterns(a, computed_nan) != _patterns(b, computed_nan))
    return f"{len(bad)} entries differ, first at {bad[:limit].tolist()}"
