"""What tests/test_oracle_reductions.py and tests/test_gpu_reductions.py share: NumPy restatements of the reductions of operators/misc.c and, as
plain Python, the launch arithmetic of kernels/blas1.hip (hpgmg_hip_norm_max, ordered_sum) and kernels/reduce.hip (final_max_kernel) that decides
which kernel and which trip of which loop a cell meets.  The GPU tests assert the path they claim against these plans, so a later change of a
constant there fails loudly instead of silently moving an edge away from the case that was placed on it.

A "geometry" is (boxes per side, box side); a "field" a (boxes, volume) array of whole padded boxes, as Level.read_all() returns it.
"""
from collections import namedtuple

import numpy as np

HUGE = 1.0e6                    # the planted maximum; everything else is in [-1, 1]
TILE_J = TILE_K = 8             # BLOCKCOPY_TILE_J / _K: a tile of the sums is side x 8 x 8 cells
ROWS_PER_BLOCK = 4              # kRowsPerBlock: 256 lanes = 4 waves = 4 rows
SMALL_NORM_BLOCKS = 64          # nblk <= 64: absmax_small_kernel
MAX_NORM_BLOCKS = 4096          # per_box is halved while per_box * boxes exceeds it
ROWS_IN_FLIGHT = 4              # absmax_rows: rows row0 + u * waves, u = 0 .. 3
FINAL_MAX_LANES = 256           # final_max_kernel: four loads (t, t + 256, t + 512, t + 768) per lane and trip, then a tail of single loads
SMALL_SUM_TILES = 64            # ntiles <= 64: tile_sum_kernel<true>, one launch
SUM_GROUP = 8                   # kSumGroup: rows a wave fetches together
SUM_MAX_CHUNKS = 8              # kSumMaxChunks: rows of up to 512 cells


def ceil_div(a, b):
    return -(-a // b)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------- cells of a level
def cell_offsets(level):
    """(side, side, side) array, (k, j, i) order, of the raw offsets of a box's interior cells."""
    d, g = level.box_dim, level.ghosts
    k, j, i = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
    return (i + g) + (j + g) * level.jStride + (k + g) * level.kStride


def interior(level, field):
    """(boxes, side, side, side) copy, (k, j, i) order, of the interior cells of a field."""
    return field[:, cell_offsets(level)]


def random_field(level, seed):
    """Whole padded boxes in [-1, 1): ghost cells and padding carry values too, so a reduction that reads one cell too many shows."""
    return np.random.default_rng(seed).random((level.num_boxes, level.volume)) * 2.0 - 1.0


# ---------------------------------------------------------------------------------------------------------------------------- restatements
def chain(x):
    """A strict left-to-right sum starting from 0.0 (np.add.accumulate is sequential; np.sum is pairwise)."""
    return np.add.accumulate(np.concatenate(([0.0], np.asarray(x, dtype=np.float64).ravel())))[-1]


def tile_partials(level, a, b=None):
    """misc.c:261-269 as the oracle and tile_sum_kernel do it: one partial per side x 8 x 8 tile, tiles numbered box-major, then k tile, then j tile;
    a partial is the chain over the tile's cells in k, j, i order.  Products are formed first."""
    x = interior(level, a)
    if b is not None:
        x = x * interior(level, b)
    d = level.box_dim
    return np.array([chain(x[box, k0:k0 + TILE_K, j0:j0 + TILE_J, :])
                     for box in range(level.num_boxes) for k0 in range(0, d, TILE_K) for j0 in range(0, d, TILE_J)])


def tile_sum(level, a, b=None, partials=tile_partials):
    """dot(a, b), or the sum of a: the partials chained in tile order."""
    return chain(partials(level, a, b))


def mean_of(level, total):
    n = float(level.dim)
    return total / (n * n * n)


def abs_max(level, a, nan=False):
    x = np.abs(interior(level, a))
    return np.nanmax(x) if nan else x.max()


# ---------------------------------------------------------------------------------------------------------------------------- element-wise passes
EW_VECTORS = 10                 # the calls below name vectors 0 .. 9, as test_gpu_operators.test_blas1_and_reductions does


def elementwise_fields(level, seed):
    """Seeded content of the ten vectors; vector 5 (the divisor of invert_vector) is kept away from zero."""
    init = [random_field(level, seed + v) for v in range(EW_VECTORS)]
    init[5] = np.abs(init[5]) + 0.5
    return init


def elementwise_calls(lv):
    L = lv.b.lib
    L.add_vectors(lv.ptr, 0, 0.75, 1, -1.25, 2)
    L.mul_vectors(lv.ptr, 3, 2.0, 1, 2)
    L.invert_vector(lv.ptr, 4, 3.0, 5)
    L.scale_vector(lv.ptr, 1, -0.5, 2)
    L.shift_vector(lv.ptr, 2, 2, 0.125)
    L.zero_vector(lv.ptr, 6)
    L.init_vector(lv.ptr, 7, 2.5)
    L.color_vector(lv.ptr, 8, 3, 1, 2, 0)
    L.random_vector(lv.ptr, 9)


def elementwise_expected(level, init):
    """What elementwise_calls() leaves in whole padded boxes: one NumPy operation per operation of the kernel, in its association
    (sa * a * b is (sa * a) * b); interior cells only, except zero_vector / init_vector, which also clear the ghost cells (not the row padding)."""
    d, g = level.box_dim, level.ghosts
    q = cell_offsets(level)
    v = [x[:, q] for x in init]
    out = [x.copy() for x in init]
    out[0][:, q] = 0.75 * v[1] + (-1.25) * v[2]
    out[3][:, q] = (2.0 * v[1]) * v[2]
    out[4][:, q] = 3.0 / v[5]
    out[1][:, q] = -0.5 * v[2]
    out[2][:, q] = v[2] + 0.125
    w = d + 2 * g
    k, j, i = np.meshgrid(np.arange(w), np.arange(w), np.arange(w), indexing="ij")
    padded = i + j * level.jStride + k * level.kStride
    out[6][:, padded] = 0.0
    out[7][:, padded] = 0.0
    out[7][:, q] = 2.5
    k, j, i = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
    for box in range(level.num_boxes):
        li, lj, lk = level.box_low(box)
        si, sj, sk = ((i + li + 1) % 3 == 0) * 1.0, ((j + lj + 2) % 3 == 0) * 1.0, ((k + lk + 0) % 3 == 0) * 1.0
        out[8][box, q] = si * sj * sk
    out[9][:, q] = -1.000 + 2.0 * (i ^ j ^ k ^ 0x1).astype(np.float64)            # misc.c:500
    return out


# ---------------------------------------------------------------------------------------------------------------------------- launch arithmetic
NormPlan = namedtuple("NormPlan", "boxes side rows nblk path per_box halvings waves rows_in_flight row0_trips partials divide lane_trips")
SumPlan = namedtuple("SumPlan", "boxes side tiles_side ntiles kernel chunks live_chunks last_chunk_lanes lds_bytes tile_rows groups tail")


def norm_plan(boxes_per_side, side):
    """hpgmg_hip_norm_max: which kernel, and the grid of absmax_kernel."""
    boxes, rows = boxes_per_side ** 3, side * side
    nblk = ceil_div(boxes * rows, ROWS_PER_BLOCK)
    divide = (side & (side - 1)) != 0                    # absmax_rows: sh = -1
    lane_trips = ceil_div(side, 64)
    if nblk <= SMALL_NORM_BLOCKS:
        return NormPlan(boxes, side, rows, nblk, "absmax_small", 0, 0, ROWS_PER_BLOCK, 1, ceil_div(boxes * rows, ROWS_PER_BLOCK), 0, False, lane_trips)
    per_box, halvings = ceil_div(rows, ROWS_PER_BLOCK), 0
    while per_box > 1 and per_box * boxes > MAX_NORM_BLOCKS:
        per_box, halvings = (per_box + 1) // 2, halvings + 1
    waves = per_box * ROWS_PER_BLOCK
    return NormPlan(boxes, side, rows, nblk, "absmax_kernel", per_box, halvings, waves, min(ROWS_IN_FLIGHT, ceil_div(rows, waves)),
                    ceil_div(rows, ROWS_IN_FLIGHT * waves), per_box * boxes, divide, lane_trips)


def final_max_plan(n):
    """final_max_kernel over n partials: (lanes that enter the 4-way loop, its trips for lane 0, partials left to the tail loop)."""
    lanes = max(0, min(FINAL_MAX_LANES, n - 3 * FINAL_MAX_LANES))
    trips = 0
    t = 0
    while t + 3 * FINAL_MAX_LANES < n:
        trips, t = trips + 1, t + 4 * FINAL_MAX_LANES
    four_way = sum(4 * len(range(q, max(q, n - 3 * FINAL_MAX_LANES), 4 * FINAL_MAX_LANES)) for q in range(FINAL_MAX_LANES))
    return lanes, trips, n - four_way


def sum_plan(boxes_per_side, side):
    """ordered_sum: which kernel, and what a tile's wave meets."""
    boxes = boxes_per_side ** 3
    tiles_side = ceil_div(side, TILE_J)
    ntiles = tiles_side * tiles_side * boxes
    if ntiles <= SMALL_SUM_TILES:
        kernel, chunks = "tile_sum<true>", 0
    elif side <= 128:
        kernel, chunks = "wave<2>", 2
    elif side <= 256:
        kernel, chunks = "wave<4>", 4
    elif side <= 64 * SUM_MAX_CHUNKS:
        kernel, chunks = "wave<8>", SUM_MAX_CHUNKS
    else:
        kernel, chunks = "tile_sum<false>", 0
    live = ceil_div(side, 64)
    edge = side - TILE_J * (tiles_side - 1)                # j (and k) extent of the last tile of a side
    tile_rows = sorted({a * b for a in (min(side, TILE_K), edge) for b in (min(side, TILE_J), edge)}, reverse=True)
    return SumPlan(boxes, side, tiles_side, ntiles, kernel, chunks, live, side - 64 * (live - 1), 2 * SUM_GROUP * side * 8 if chunks else 0,
                   tile_rows, [ceil_div(r, SUM_GROUP) for r in tile_rows], ntiles % 64)
