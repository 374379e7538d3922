"""What tests/test_oracle_transfers.py and tests/test_gpu_transfers.py share: the rows at which the transfer kernels of kernels/blocks.hip
(restrict_blocks_kernel, restrict_cell_zero_kernel, interp_blocks_kernel, interp_tensor_kernel) are held to the oracle, the launch facts of each row
-- read off the level and its block lists through hpgmg_level_list_entry, never written down as literals --, NumPy restatements of the restrictions and
of the 7-point plugin's two interpolations in the reference's summation order, and the special-value fields of the `prescale == 0` rule.

A "geometry" is (boxes per side, box side) of the fine level; a "field" a (boxes, volume) array of whole padded boxes, as Level.read_all() returns
it.  A "plugin" is one of PLUGINS; its interpolation orders (V-cycle, F-cycle) are those of operators_hip.c: 0 piecewise constant, 1 trilinear,
2 / 3 / 4 the tensor rules p2 / v2 / v4.

Every row states the edge it exists for as a predicate over its Facts; check_row() asserts it, on the CPU, so a later change of a tile size, of the
coarsening ladder or of a constant of a launcher fails loudly instead of silently moving the edge away from the row that was placed on it.
"""
import ctypes
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import as_strided

import hpgmg_amd as H
from hpgmg_testlib import VARIANTS, Level, seeded_field
from reduction_lib import bits, ceil_div

ZERO_CHUNK = 4096               # restrict_cell_zero_kernel: doubles a zeroing workgroup clears
WAVE = 64
ROWS_PER_PASS = 4               # 256 lanes = 4 waves: coarse rows (units) a workgroup takes per pass
SLAB_ENTRIES = 4096             # hpgmg_hip_interpolate_blocks: slabs = n >= 4096 ? 1 : min(64, 4096 / n)
MAX_SLABS = 64
KC = 8                          # interp_tensor_kernel: coarse planes a unit marches over
LANES = 256

# plugin -> (configuration, (a, b) of MGBuild, order of interpolation_vcycle, order of interpolation_fcycle)
PLUGINS = {"7pt": ("7pt-cheby-helm", (1.0, 1.0), 0, 1),
           "27pt": ("27pt-cheby", (0.0, 1.0), 2, 2),
           "fv2": ("fv2-cheby", (0.0, 1.0), 3, 3),
           "fv4": ("fv4-gsrb", (0.0, 1.0), 3, 4)}
# the vector each restriction type is fed from: a cell-centred one, and the face-centred coefficients (whose ghost copies Hierarchy has exchanged)
SOURCE_OF = {H.RESTRICT_CELL: H.VECTOR_F, H.RESTRICT_FACE_I: H.VECTOR_BETA_I, H.RESTRICT_FACE_J: H.VECTOR_BETA_J, H.RESTRICT_FACE_K: H.VECTOR_BETA_K}
TYPES = (H.RESTRICT_CELL, H.RESTRICT_FACE_I, H.RESTRICT_FACE_J, H.RESTRICT_FACE_K)
PRESCALES = (0.0, 1.0, -1.0, 0.3)


# ---------------------------------------------------------------------------------------------------------------------------- hierarchies
class Hierarchy:
    """A fine level of one backend with seeded vectors and positive coefficients, and the hierarchy MGBuild puts under it (as
    test_gpu_operators.test_restriction_and_interpolation builds it).  Face-centred data is shared by two boxes -- the high face of one is the low
    face of the next --, so the ghost copies of the coefficient vectors are exchanged before MGBuild restricts them: a coarse face then has two
    agreeing writers."""

    def __init__(self, be, plugin, geom):
        self.be, self.plugin, self.geom = be, plugin, geom
        self.variant, (a, b), self.order_v, self.order_f = PLUGINS[plugin]
        self.configure()
        self.fine = be.level(*geom)
        for vid in range(self.fine.num_vectors):
            d = seeded_field(self.fine, 900 + vid)
            self.fine.write_all(vid, np.abs(d) + 0.5 if vid >= H.VECTOR_DINV else d)
        for vid in range(H.VECTOR_DINV, self.fine.num_vectors):
            be.lib.exchange_boundary(self.fine.ptr, vid, H.STENCIL_SHAPE_BOX)
        self.mg = be.lib.hpgmg_mg_create(self.fine.ptr, a, b, 1)
        assert be.lib.hpgmg_mg_num_levels(self.mg) >= 2, (plugin, geom)
        self.coarse = Level(be, be.lib.hpgmg_mg_level(self.mg, 1))

    def configure(self):
        self.be.configure(**VARIANTS[self.variant])

    def destroy(self):
        if self.mg:
            self.be.lib.hpgmg_mg_destroy(self.mg)
            self.fine.destroy()
            self.mg = None


class Hierarchies:
    """hierarchies.get(plugin, geom) -> one Hierarchy per backend, built when first asked for and kept until another row is asked for (the rows of
    one geometry follow each other in every table, and the largest hold 200 MB a side)."""

    def __init__(self, *backends):
        self.backends, self.key, self.held = backends, None, ()

    def get(self, plugin, geom):
        if self.key != (plugin, geom):
            self.close()
            self.held = tuple(Hierarchy(be, plugin, geom) for be in self.backends)
            self.key = (plugin, geom)
        for h in self.held:
            h.configure()
        return self.held

    def close(self):
        for h in self.held:
            h.destroy()
        self.key, self.held = None, ()


def pair_of(hierarchies, plugin, geom):
    """(HIP hierarchy, oracle hierarchy) of a row from a Hierarchies(hip, oracle)."""
    hh, ho = hierarchies.get(plugin, geom)
    assert (hh.be.name, ho.be.name) == ("hip", "oracle")
    assert hh.be.lib.hpgmg_mg_num_levels(hh.mg) == ho.be.lib.hpgmg_mg_num_levels(ho.mg)
    for a, b in ((hh.fine, ho.fine), (hh.coarse, ho.coarse)):
        assert a.info == b.info
    return hh, ho


# ---------------------------------------------------------------------------------------------------------------------------- block lists
Entry = namedtuple("Entry", "di dj dk rbox ri rj rk wbox wi wj wk")


def entries(level, which, idx=0, phase=1):
    """The entries of a block list of a level (which: 1 restriction[idx], 2 interpolation), phase 1 = the copies between local boxes."""
    lib, counts, out, found = level.b.lib, (ctypes.c_int * 3)(), (ctypes.c_int * 11)(), []
    assert lib.hpgmg_level_list_counts(level.ptr, which, idx, counts) == 0, "messages on a one-rank level"
    assert counts[0] == 0 and counts[2] == 0
    for n in range(counts[phase]):
        assert lib.hpgmg_level_list_entry(level.ptr, which, idx, phase, n, out) == 0
        found.append(Entry(*out))
    assert lib.hpgmg_level_list_entry(level.ptr, which, idx, phase, counts[phase], out) == -1
    return found


def restriction_entries(h, rtype):
    return entries(h.fine, 1, rtype)          # the send side hangs off the fine level


def interpolation_entries(h):
    return entries(h.coarse, 2)               # the send side hangs off the coarse level


# ---------------------------------------------------------------------------------------------------------------------------- launch facts
Facts = namedtuple("Facts", "fine_boxes coarse_boxes boxes_in_i "
                            "r_entries r_cells r_di r_tiles r_offsets "
                            "i_entries slabs ci_n cj_n ck_n wci rpw idle_lanes row_groups_past rows passes second_pass "
                            "coarse_volume coarse_ghosts chunks last_chunk")


def wci_of(ci_n):
    return 64 if ci_n > 32 else 32 if ci_n > 16 else 16 if ci_n > 8 else 8


def facts_of(h):
    """The launch facts of a row from its hierarchy.
    restriction (restrict_blocks_kernel, one workgroup of 256 lanes per entry, lane t takes cells t, t + 256, ...):
      r_entries[type] entries; r_cells[type] the set of di dj dk; r_di[type] the set of di; r_tiles the set of (dj, dk) over all four types;
      r_offsets the set of (write.i, write.j, write.k) of the cell list.
    interpolation (hpgmg_hip_interpolate_blocks: grid (entries, slabs), 4 waves per workgroup):
      i_entries, slabs; ci_n / cj_n / ck_n the sets of the entries' extents; wci / rpw of interp_tensor_kernel (sets, per ci_n);
      idle_lanes: lanes of a sub-wave past ci_n (wci - ci_n, the set); row_groups_past: an entry whose last row group of rpw rows reaches past cj_n;
      rows the most coarse rows cj_n ck_n of an entry and passes = the most passes a workgroup of interp_blocks_kernel makes over them;
      second_pass: a coarse row longer than a wave (the `ci += 64` pass).
    restrict_cell_zero_kernel: chunks of 4096 doubles per coarse box of coarse_volume doubles, last_chunk the length of the last."""
    f, c = h.fine, h.coarse
    R = {t: restriction_entries(h, t) for t in TYPES}
    I = interpolation_entries(h)
    n = len(I)
    slabs = 1 if n >= SLAB_ENTRIES else min(MAX_SLABS, SLAB_ENTRIES // n)
    ci = {e.di for e in I}
    rows = max(e.dj * e.dk for e in I)
    chunks = ceil_div(c.volume, ZERO_CHUNK)
    return Facts(fine_boxes=f.num_boxes, coarse_boxes=c.num_boxes, boxes_in_i=f.info[H.INFO_BOXES_IN_I],
                 r_entries={t: len(R[t]) for t in TYPES}, r_cells={t: {e.di * e.dj * e.dk for e in R[t]} for t in TYPES},
                 r_di={t: {e.di for e in R[t]} for t in TYPES}, r_tiles={(e.dj, e.dk) for t in TYPES for e in R[t]},
                 r_offsets={(e.wi, e.wj, e.wk) for e in R[H.RESTRICT_CELL]},
                 i_entries=n, slabs=slabs, ci_n=ci, cj_n={e.dj for e in I}, ck_n={e.dk for e in I},
                 wci={wci_of(x) for x in ci}, rpw={WAVE // wci_of(x) for x in ci}, idle_lanes={wci_of(x) - x for x in ci if x <= WAVE},
                 row_groups_past=any(e.dj % (WAVE // wci_of(e.di)) for e in I), rows=rows, passes=ceil_div(rows, slabs * ROWS_PER_PASS),
                 second_pass=max(ci) > WAVE,
                 coarse_volume=c.volume, coarse_ghosts=c.ghosts, chunks=chunks, last_chunk=c.volume - ZERO_CHUNK * (chunks - 1))


# ---------------------------------------------------------------------------------------------------------------------------- the rows
Row = namedtuple("Row", "plugin geom edge holds")
_C, _I, _J, _K = TYPES


def _tile(f, dj, dk=None):
    return any(a == dj and (dk is None or b == dk) for a, b in f.r_tiles) or any(b == dj and (dk is None or a == dk) for a, b in f.r_tiles)


RESTRICTION_ROWS = [
    Row("7pt", (1, 2), "one cell: fewer cells than the 256 lanes", lambda f: f.r_cells[_C] == {1} and max(f.r_cells[_I]) < LANES),
    Row("7pt", (3, 4), "a middle box on no wall; di = 3", lambda f: f.boxes_in_i >= 3 and f.r_di[_I] == {3}),
    Row("7pt", (4, 8), "8 fine boxes merged into one coarse box at an offset; di = 5",
        lambda f: f.fine_boxes == 8 * f.coarse_boxes and len(f.r_offsets) == 8 and (4, 4, 4) in f.r_offsets and f.r_di[_I] == {5}),
    Row("7pt", (1, 12), "n = 216 and 252: below 256 and no multiple of it; di = 7", lambda f: f.r_cells[_C] == {216} and f.r_cells[_I] == {252}),
    Row("7pt", (2, 20), "di = 11; J / K tiles 8 + 2 and 8 + 3; n no multiple of 256",
        lambda f: f.r_di[_I] == {11} and _tile(f, 2) and _tile(f, 3) and all(n % LANES for n in f.r_cells[_I])),
    Row("7pt", (1, 24), "di = 13; J / K tiles 8 + 4 and 8 + 5", lambda f: f.r_di[_I] == {13} and _tile(f, 8, 4) and _tile(f, 5)),
    Row("7pt", (1, 64), "di = 33; J / K tiles 8 + 1; n above 256", lambda f: f.r_di[_I] == {33} and _tile(f, 8, 1) and _tile(f, 1, 8) and max(f.r_cells[_C]) > LANES),
    Row("7pt", (1, 128), "di = 65: a row longer than a wave; J / K tiles 8 + 1", lambda f: f.r_di[_I] == {65} and _tile(f, 8, 1)),
    Row("fv4", (2, 8), "ghost depth 2; 8 boxes merged", lambda f: f.coarse_ghosts == 2 and f.fine_boxes == 8 * f.coarse_boxes),
    Row("fv4", (1, 64), "ghost depth 2; di = 33", lambda f: f.coarse_ghosts == 2 and f.r_di[_I] == {33}),
    Row("27pt", (2, 8), "8 boxes merged", lambda f: f.fine_boxes == 8 * f.coarse_boxes and f.coarse_ghosts == 1),
    Row("27pt", (1, 64), "di = 33", lambda f: f.r_di[_I] == {33} and _tile(f, 8, 1)),
]

RESTRICT_ZERO_ROWS = [
    Row("7pt", (2, 8), "one coarse box of fewer than 4096 doubles: one short chunk", lambda f: f.coarse_boxes == 1 and f.chunks == 1 and f.last_chunk < ZERO_CHUNK),
    Row("7pt", (4, 8), "several coarse boxes, one short chunk each", lambda f: f.coarse_boxes == 8 and f.chunks == 1 and f.last_chunk < ZERO_CHUNK),
    Row("7pt", (1, 32), "two chunks, a short last one", lambda f: f.chunks == 2 and f.last_chunk < ZERO_CHUNK),
    Row("7pt", (2, 32), "several coarse boxes of several chunks, a short last one", lambda f: f.coarse_boxes == 8 and f.chunks >= 2 and f.last_chunk < ZERO_CHUNK),
    Row("7pt", (1, 64), "many chunks, a short last one", lambda f: f.chunks >= 8 and f.last_chunk < ZERO_CHUNK),
    Row("fv4", (2, 16), "ghost depth 2, several coarse boxes", lambda f: f.coarse_ghosts == 2 and f.coarse_boxes == 8 and f.last_chunk < ZERO_CHUNK),
]

_WIDE = ("27pt", "fv2", "fv4")
# (1, 12) ... (1, 72): coarse rows of 6, 12, 20, 36 -- a sub-wave of 8, 16, 32, 64 lanes, each with idle lanes.  Which plugins take them: RAGGED_WIDE
_RAGGED = [((1, 12), "wci = 8 with 2 idle lanes; rpw = 8 rows, 6 live", lambda f: f.wci == {8} and f.idle_lanes == {2} and f.row_groups_past),
           ((1, 24), "wci = 16 with 4 idle lanes; tiles of 8 and 4 rows", lambda f: f.wci == {16} and f.idle_lanes == {4} and f.cj_n == {8, 4}),
           ((1, 40), "wci = 32 with 12 idle lanes; tiles of 8 and 4 rows", lambda f: f.wci == {32} and f.idle_lanes == {12} and f.cj_n == {8, 4}),
           ((1, 72), "wci = 64 with 28 idle lanes; tiles of 8 and 4 rows", lambda f: f.wci == {64} and f.idle_lanes == {28} and f.cj_n == {8, 4})]
RAGGED_WIDE = _WIDE             # plugins whose ragged rows run: all three (see the docstring of tests/test_gpu_transfers.py)
RAGGED_ROWS = [Row(p, g, e, ok) for p in _WIDE for g, e, ok in _RAGGED]         # all of them: their predicates are checked on the oracle in any case

INTERPOLATION_ROWS = [
    Row("7pt", (1, 2), "one coarse cell", lambda f: f.ci_n == {1} and f.rows == 1),
    Row("7pt", (3, 4), "27 entries of 2 x 2 x 2; a middle box", lambda f: f.ci_n == {2} and f.i_entries == 27 and f.slabs == MAX_SLABS),
    Row("7pt", (4, 8), "64 entries: slabs = 64 of 16 rows, most workgroups idle", lambda f: f.i_entries == 64 and f.slabs == 64 and f.rows == 16),
    Row("7pt", (1, 12), "ci_n = 6, ragged; one entry of 36 rows", lambda f: f.ci_n == {6} and f.i_entries == 1 and f.rows == 36),
    Row("7pt", (2, 20), "ci_n = 10; tiles of 8 and 2 rows", lambda f: f.ci_n == {10} and f.cj_n == {8, 2}),
    Row("7pt", (1, 40), "ci_n = 20; tiles of 8 and 4", lambda f: f.ci_n == {20} and f.cj_n == {8, 4}),
    Row("7pt", (1, 136), "ci_n = 68: the second `ci += 64` pass with 4 live lanes", lambda f: f.ci_n == {68} and f.second_pass),
    Row("7pt", (16, 4), "4096 entries: slabs == 1", lambda f: f.i_entries == 4096 and f.slabs == 1 and f.fine_boxes == 4096),
] + [Row(p, g, e, ok) for p in _WIDE for g, e, ok in [
    ((2, 8), "wci = 8, rpw = 8: 4 lanes of 8 and 4 rows of 8 live", lambda f: f.wci == {8} and f.rpw == {8} and f.idle_lanes == {4} and f.row_groups_past),
    ((2, 16), "wci = 8, rpw = 8, full", lambda f: f.wci == {8} and f.idle_lanes == {0} and not f.row_groups_past),
    ((1, 32), "wci = 16, rpw = 4", lambda f: f.wci == {16} and f.rpw == {4}),
    ((1, 64), "wci = 32, rpw = 2", lambda f: f.wci == {32} and f.rpw == {2}),
    ((1, 128), "wci = 64, rpw = 1; 64 entries of 8 units over 64 slabs", lambda f: f.wci == {64} and f.rpw == {1} and f.i_entries == 64)]
] + [r for r in RAGGED_ROWS if r.plugin in RAGGED_WIDE] + [
    # the tensor kernel's own `ci += wci` pass: a coarse row longer than its widest sub-wave (orders 2, and 3 and 4)
    Row(p, (1, 136), "ci_n = 68 > wci = 64: the second `ci += wci` pass with 4 live lanes", lambda f: f.ci_n == {68} and f.wci == {64} and f.second_pass)
    for p in ("27pt", "fv4") if p in RAGGED_WIDE]

# one small and one >= 64 row per order 0 ... 4 (7pt: orders 0 and 1; 27pt: 2; fv2: 3; fv4: 3 and 4)
SPECIAL_ROWS = [Row(p, g, "prescale == 0 on the special-value fields", lambda f: True) for p in ("7pt", "27pt", "fv2", "fv4") for g in ((2, 16), (1, 64))]

ZERO_INTERPOLATION_ROWS = [Row("7pt", (2, 16), "order 17, 8 entries a box", lambda f: f.ci_n == {8}),
                           Row("7pt", (1, 40), "order 17, ragged", lambda f: f.ci_n == {20})] + \
                          [Row(p, g, e, ok) for p in _WIDE for g, e, ok in [((2, 16), "zeroed tensor form, wci = 8", lambda f: f.wci == {8}),
                                                                            ((1, 64), "zeroed tensor form, wci = 32", lambda f: f.wci == {32})]]

TABLES = {"restriction": RESTRICTION_ROWS, "restrict_zero": RESTRICT_ZERO_ROWS, "interpolation": INTERPOLATION_ROWS, "special": SPECIAL_ROWS,
          "zero_interpolation": ZERO_INTERPOLATION_ROWS}


def row_id(row):
    return f"{row.plugin}-{row.geom[0]}x{row.geom[1]}"


def check_row(row, h):
    """The row's edge, from the hierarchy's own lists; returns the facts."""
    f = facts_of(h)
    assert (h.plugin, h.geom) == (row.plugin, row.geom)
    assert row.holds(f), (row_id(row), row.edge, f)
    return f


# ---------------------------------------------------------------------------------------------------------------------------- fields
def same_bits(a, b):
    """np.array_equal on bits, every NaN counted as the one NaN (0 * Inf is -NaN on one machine and +NaN on another)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(np.where(np.isnan(a), np.nan, a)), bits(np.where(np.isnan(b), np.nan, b)))


def differing(a, b):
    """For a failure message: how many cells differ, and the first few (box, offset)."""
    bad = bits(np.where(np.isnan(a), np.nan, a)) != bits(np.where(np.isnan(b), np.nan, b))
    return f"{int(bad.sum())} cells differ, first at {np.argwhere(bad)[:4].tolist()}"


def box_views(level, field):
    """(boxes, w, w, w) writable view of a field, [box, k, j, i] over interior and ghost cells (w = side + 2 ghosts); the padding is not in it."""
    w, s = level.box_dim + 2 * level.ghosts, field.strides[-1]
    assert field.shape == (level.num_boxes, level.volume) and field.flags.c_contiguous
    return as_strided(field, shape=(level.num_boxes, w, w, w), strides=(field.strides[0], level.kStride * s, level.jStride * s, s))


def interior_of(level, field):
    g, d = level.ghosts, level.box_dim
    return box_views(level, field)[:, g:g + d, g:g + d, g:g + d]


def nan_field(level):
    return np.full((level.num_boxes, level.volume), np.nan)


def global_to_field(level, cells, fill):
    """A field whose interiors hold the global (k, j, i) array `cells` and every other cell what `fill` (a field) holds."""
    out, d, g = fill.copy(), level.box_dim, level.ghosts
    v = box_views(level, out)
    for b in range(level.num_boxes):
        li, lj, lk = level.box_low(b)
        v[b, g:g + d, g:g + d, g:g + d] = cells[lk:lk + d, lj:lj + d, li:li + d]
    return out


CUBE = 7                        # side of the two cubes of zeros: 3^3 cells of each see only zeros even at radius 2


def coarse_special(level, seed):
    """Random, except two cubes of CUBE^3 cells: global cells [1, 1 + CUBE)^3 hold +0.0, [n - 1 - CUBE, n - 1)^3 hold -0.0."""
    n = level.dim
    assert n >= 2 * CUBE + 2 and CUBE >= 5
    cells = np.random.default_rng(seed).random((n, n, n)) * 2.0 - 1.0
    cells[1:1 + CUBE, 1:1 + CUBE, 1:1 + CUBE] = 0.0
    cells[n - 1 - CUBE:n - 1, n - 1 - CUBE:n - 1, n - 1 - CUBE:n - 1] = -0.0
    return global_to_field(level, cells, seeded_field(level, seed + 1))


KINDS = ("+0", "-0", "positive", "negative", "nan", "inf")


def old_special(level):
    """A fine "old" field that cycles through +0.0, -0.0, a positive number, a negative number, NaN and +Inf: cell q of a padded box (ghosts and
    padding too) holds kind (q + q // 6) % 6 -- the second term moves the cycle on by one every six cells, so that the eight children of a coarse
    cell, which lie at q, q + 1, q + jStride ... with even strides, do not all meet the same two kinds.  Returns (field, kind index per offset)."""
    q = np.arange(level.volume)
    kind = (q + q // 6) % 6
    values = np.array([0.0, -0.0, 1.25, -2.5, np.nan, np.inf])
    mag = np.where(kind >= 2, 1.0 + (q % 7) / 8.0, 1.0)
    field = np.tile(values[kind] * mag, (level.num_boxes, 1))
    assert np.signbit(field[0, kind == 1]).all() and not np.signbit(field[0, kind == 0]).any()
    return field, kind


def expected_at_prescale_zero(exact, clean, old):
    """The stated exception, and nothing wider: the kernels fetch the old value only where the result is a zero, so a non-finite old value is dropped
    where the interpolant is not a zero (the reference gives 0 * NaN = NaN there).  exact: the oracle onto `old`; clean: the oracle onto zeros."""
    dropped = ~np.isfinite(old) & (clean != 0.0)
    return np.where(dropped, clean, exact), dropped


def class_counts(exact, clean, old_kind_of_cell, cells):
    """Over the interior `cells` (offsets): {(result class, old kind): count} with result class "+0" / "-0" (a zero result, by sign), "nan" (a NaN
    result where the interpolant is a zero), "value" (the interpolant is not a zero)."""
    out = {}
    e, c, k = exact[:, cells].ravel(), clean[:, cells].ravel(), np.tile(old_kind_of_cell[cells].ravel(), exact.shape[0])
    zero_interp = c == 0.0
    for name, mask in (("+0", (e == 0.0) & ~np.signbit(e)), ("-0", (e == 0.0) & np.signbit(e)), ("nan", np.isnan(e) & zero_interp), ("value", ~zero_interp)):
        for kk, kind in enumerate(KINDS):
            out[name, kind] = int((mask & (k == kk)).sum())
    return out


def reachable_classes(order):
    """What the special-value fields must produce at `order`, from the arithmetic alone.  Inside a cube every neighbour of a child is the same zero z.
    Order 0 gives the interpolant y = z; order 1 a sum of positive multiples of z, = z.  v2 (order 3) is c1 +- (1/8) (c0 - c2): the difference of equal
    zeros is +0.0, so the odd child of z = -0.0 is (-0.0) - (+0.0) = -0.0 and the child that is odd in i, j and k keeps it; the even child is
    (-0.0) + (+0.0) = +0.0.  p2 (order 2) adds w2 z with w2 < 0 and v4 (order 4) subtracts c2 (+0.0) with c2 < 0, a -0.0: both give +0.0 in both cubes.
    Then v = 0 * old + y: old finite gives (+-0) + y, which is -0.0 only if both are -0.0, that is y = -0.0 and old in {-0.0, negative}; old = NaN or Inf
    gives NaN.  Outside the cubes y is not a zero ("value"), over every kind."""
    want = [("+0", k) for k in ("+0", "-0", "positive", "negative")] + [("nan", "nan"), ("nan", "inf")] + [("value", k) for k in KINDS]
    if order in (0, 1, 3):
        want += [("-0", "-0"), ("-0", "negative")]
    return want


# ---------------------------------------------------------------------------------------------------------------------------- restatements
def restrict_np(rtype, lists, Lf, fine, Lc, coarse, wrong=None):
    """restriction.c:49-91 over a list of entries, fp64, one rounding per operation, in the reference's order: returns the coarse field, `coarse`
    with the cells the list names overwritten.  wrong="cell-order": the cell sum as a tree of pairs; wrong="face-pairs": face I averaged over
    the J pair alone, the K pair left out (f[0] + f[rj] taken twice)."""
    out = coarse.copy()
    F, C, gf, gc = box_views(Lf, fine), box_views(Lc, out), Lf.ghosts, Lc.ghosts
    for e in lists:
        def f(oi, oj, ok):
            return F[e.rbox, gf + e.rk + ok:gf + e.rk + ok + 2 * e.dk:2, gf + e.rj + oj:gf + e.rj + oj + 2 * e.dj:2, gf + e.ri + oi:gf + e.ri + oi + 2 * e.di:2]
        if rtype == H.RESTRICT_CELL:
            if wrong == "cell-order":
                v = ((f(0, 0, 0) + f(1, 0, 0)) + (f(0, 1, 0) + f(1, 1, 0))) + ((f(0, 0, 1) + f(1, 0, 1)) + (f(0, 1, 1) + f(1, 1, 1)))
            else:
                v = f(0, 0, 0) + f(1, 0, 0)
                for o in ((0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                    v = v + f(*o)
            v = v * 0.125
        else:
            terms = {H.RESTRICT_FACE_I: ((0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)), H.RESTRICT_FACE_J: ((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1)),
                     H.RESTRICT_FACE_K: ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0))}[rtype]
            if wrong == "face-pairs" and rtype == H.RESTRICT_FACE_I:
                terms = ((0, 0, 0), (0, 1, 0), (0, 0, 0), (0, 1, 0))
            v = f(*terms[0]) + f(*terms[1])
            v = v + f(*terms[2])
            v = v + f(*terms[3])
            v = v * 0.25
        C[e.wbox, gc + e.wk:gc + e.wk + e.dk, gc + e.wj:gc + e.wj + e.dj, gc + e.wi:gc + e.wi + e.di] = v
    return out


def interpolate_np(order, lists, Lf, fine, prescale, Lc, coarse, wrong=None):
    """interpolation_p0.c:43 (order 0) and interpolation_p1.c:40-70 (order 1) over a list of entries: returns the fine field.  `coarse` holds the ghost
    cells as the operator's exchange and boundary condition left them.  Order 1 adds the eight weighted terms in the order of interp_blocks_kernel's
    blend, which is the reference's: centre, k, j, jk, i, ik, ij, ijk.  wrong="swap-ik": the roles of the i and k neighbours swapped."""
    out = fine.copy()
    F, C, gf, gc = box_views(Lf, out), box_views(Lc, coarse), Lf.ghosts, Lc.ghosts
    for e in lists:
        def c(oi, oj, ok):
            return C[e.rbox, gc + e.rk + ok:gc + e.rk + ok + e.dk, gc + e.rj + oj:gc + e.rj + oj + e.dj, gc + e.ri + oi:gc + e.ri + oi + e.di]
        for fk in (0, 1):
            for fj in (0, 1):
                for fi in (0, 1):
                    w = F[e.wbox, gf + e.wk + fk:gf + e.wk + fk + 2 * e.dk:2, gf + e.wj + fj:gf + e.wj + fj + 2 * e.dj:2, gf + e.wi + fi:gf + e.wi + fi + 2 * e.di:2]
                    v = prescale * w
                    if order == 0:
                        v = v + c(0, 0, 0)
                    else:
                        oi, oj, ok = 2 * fi - 1, 2 * fj - 1, 2 * fk - 1
                        if wrong == "swap-ik":
                            steps = ((0, 0, 0), (oi, 0, 0), (0, oj, 0), (oi, oj, 0), (0, 0, ok), (oi, 0, ok), (0, oj, ok), (oi, oj, ok))
                        else:
                            steps = ((0, 0, 0), (0, 0, ok), (0, oj, 0), (0, oj, ok), (oi, 0, 0), (oi, 0, ok), (oi, oj, 0), (oi, oj, ok))
                        for weight, o in zip((0.421875, 0.140625, 0.140625, 0.046875, 0.140625, 0.046875, 0.046875, 0.015625), steps):
                            v = v + weight * c(*o)
                    w[...] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------------- operator calls
def call_interpolation(h, which, id_f, prescale, id_c):
    fn = h.be.lib.interpolation_vcycle if which == "vcycle" else h.be.lib.interpolation_fcycle
    fn(h.fine.ptr, id_f, prescale, h.coarse.ptr, id_c)


def order_of(h, which):
    return h.order_v if which == "vcycle" else h.order_f


def run_interpolation(h, which, prescale, old, coarse_field, id_f=H.VECTOR_U, id_c=H.VECTOR_R):
    """Write the two fields, interpolate, and return (fine field, coarse field) as the operator left them."""
    h.fine.write_all(id_f, old)
    h.coarse.write_all(id_c, coarse_field)
    call_interpolation(h, which, id_f, prescale, id_c)
    return h.fine.read_all(id_f), h.coarse.read_all(id_c)


SpecialCase = namedtuple("SpecialCase", "old kind coarse exact clean expected dropped")


def special_case(ho, which):
    """The `prescale == 0` case of an oracle hierarchy: the two oracle runs and what the kernels are held to."""
    old, kind = old_special(ho.fine)
    coarse = coarse_special(ho.coarse, 77)
    exact, _ = run_interpolation(ho, which, 0.0, old, coarse)
    clean, _ = run_interpolation(ho, which, 0.0, np.zeros_like(old), coarse)
    expected, dropped = expected_at_prescale_zero(exact, clean, old)
    return SpecialCase(old, kind, coarse, exact, clean, expected, dropped)


def declare_fused(lib):
    vp, c_int = ctypes.c_void_p, ctypes.c_int
    lib.hpgmg_restrict_zero_fused.restype = c_int
    lib.hpgmg_restrict_zero_fused.argtypes = [vp, c_int, vp, c_int, c_int]
    lib.hpgmg_zero_interpolation_fcycle_fused.restype = c_int
    lib.hpgmg_zero_interpolation_fcycle_fused.argtypes = [vp, c_int, vp, c_int]
    return lib
