"""What the tests of the CG passes (include/hpgmg_operators.h hpgmg_pcg_*; kernels/pcg.hip) and of the Gram launch (kernels/gram.hip)
share: NumPy restatements of the one summation order of the header, of hpgmg_pcg_update and of matmul(), and -- as plain Python -- the launch
arithmetic of pcg.hip (pcg_grid, pcg_fold) and gram.hip that decides which lane, slot and trip a value meets.  The GPU tests assert the row of
their table against these plans (as tests/reduction_lib.py's), so a later change of a constant in the kernels fails loudly instead of silently
moving an edge away from the case that was placed on it.

A "geometry" is (boxes per side, box side); a "field" a (boxes, volume) array of whole padded boxes, as Level.read_all() returns it, boxes in level
order; a "box array" a (boxes, side, side, side) array of interior cells in (k, j, i) order (reduction_lib.interior of a field).
"""
import ctypes

import numpy as np

import hpgmg_amd as H
from reduction_lib import bits, ceil_div, cell_offsets, interior, random_field

SEGMENT, COLUMNS = 16, 256      # HPGMG_PCG_SEGMENT, HPGMG_PCG_COLUMNS of include/hpgmg_operators.h
FOLD_LANES = 1024               # kFoldLanes: the one workgroup of pcg_fold_kernel
GRAM_THREADS = 256              # kGramThreads: lanes of a box's workgroup, one (mm, nn) pair per lane and slot
GRAM_CHUNK = 64                 # kGramChunk: interior cells staged at a time
GRAM_MAX_SIDE = 32              # kGramMaxSide: rows, cols <= 32


# ---------------------------------------------------------------------------------------------------------------------------- the header's order
def fold(V):
    """V[m] = V[m] + V[m + stride] for every m that is a multiple of 2 stride, stride = 1, 2, 4, ..., over V padded with 0.0 to a power of two."""
    size = 1
    while size < V.size:
        size *= 2
    W = np.zeros(size)
    W[:V.size] = V
    while W.size > 1:
        W = W[0::2] + W[1::2]
    return float(W[0])


def header_order_dot(a, b, side, segment=SEGMENT, column_major=False, leaf_tree=True):
    """a . b of two box arrays in the order of include/hpgmg_operators.h: products first; per box B, segment s and column c = i + side j the chain
    0.0 + q(k = 16 s) + ... over the segment's planes; the chains are the leaves V[c + W (s + S B)], 0.0 where c >= side^2, folded by fold().
    The keywords state the order WRONGLY, for the tests that show the data can tell: column_major puts column (i, j) at c = j + side i; segment
    is another plane count; leaf_tree=False adds the 256 leaves of a workgroup's item one after the other and folds the items' values only."""
    q = a * b
    boxes = q.shape[0]
    assert q.shape == (boxes, side, side, side)
    W = COLUMNS * ceil_div(side * side, COLUMNS)
    S = ceil_div(side, segment)
    V = np.zeros((boxes, S, W))
    for s in range(S):
        chain = np.zeros((boxes, side, side))
        for k in range(s * segment, min(s * segment + segment, side)):
            chain = chain + q[:, k]
        if column_major:
            chain = chain.transpose(0, 2, 1)
        V[:, s, :side * side] = chain.reshape(boxes, side * side)
    if not leaf_tree:
        items = np.zeros(boxes * S * W // COLUMNS)
        for leaf in V.reshape(-1, COLUMNS).T:             # one addition per leaf, in c order: no tree below stride 256
            items = items + leaf
        return fold(items)
    return fold(V.reshape(-1))


def dense_boxes(v, side):
    """The box array of a dense (n, n, n) array [k][j][i] cut into boxes of `side`: box B = bi + nb (bj + nb bk), the level order of a Solver."""
    nb = v.shape[0] // side
    return np.stack([v[bk * side:(bk + 1) * side, bj * side:(bj + 1) * side, bi * side:(bi + 1) * side]
                     for bk in range(nb) for bj in range(nb) for bi in range(nb)])


def dot(level, fa, fb, **wrong):
    """header_order_dot of two fields of a plain level."""
    return header_order_dot(interior(level, fa), interior(level, fb), level.box_dim, **wrong)


def update(level, fx, fr, fp, fAp, alpha):
    """hpgmg_pcg_update on fields: per interior cell x = x + alpha * p, r = r - alpha * Ap (the product first), and max |r| from 0.0, a NaN never
    the maximum (`f > best` is false for it).  Ghost and padding cells keep what they held.  Returns (x, r, rmax)."""
    q = cell_offsets(level)
    x, r = fx.copy(), fr.copy()
    dx, dr = alpha * fp[:, q], alpha * fAp[:, q]
    x[:, q] = fx[:, q] + dx
    r[:, q] = fr[:, q] - dr
    return x, r, float(np.fmax.reduce(np.abs(r[:, q]).ravel(), initial=0.0))


# ---------------------------------------------------------------------------------------------------------------------------- matmul()
def gram_restated(level, id_A, id_B):
    """matmul() (kernels/gram.hip's order contract): entry (mm, nn), nn >= mm, is per box ONE chain from 0.0 over the products of the interior
    cells in k, j, i order -- a Python loop over (a * b).tolist(), nothing NumPy could reassociate --, the boxes' chains added in box order from
    0.0, the upper triangle mirrored where mm < cols and nn < rows; every other entry is 0.0."""
    rows, cols = len(id_A), len(id_B)
    V = {v: interior(level, level.read_all(v)).reshape(level.num_boxes, -1) for v in set(id_A) | set(id_B)}
    C = np.zeros(rows * cols)
    for mm in range(rows):
        for nn in range(mm, cols):
            total = 0.0
            for box in range(level.num_boxes):
                chain = 0.0
                for q in (V[id_A[mm]][box] * V[id_B[nn]][box]).tolist():
                    chain = chain + q
                total = total + chain
            C[mm * cols + nn] = total
            if mm < cols and nn < rows:
                C[nn * cols + mm] = total
    return C


# ---------------------------------------------------------------------------------------------------------------------------- launch arithmetic
def pcg_items(side, boxes):
    """pcg_grid: (column blocks of a box, segments of a box, workgroups = values the fold launch gets)."""
    ncb, nseg = ceil_div(side * side, COLUMNS), ceil_div(side, SEGMENT)
    return ncb, nseg, ncb * nseg * boxes


def pcg_fold_plan(items):
    """pcg_fold / pcg_fold_body over `items` values: (chunk: the consecutive values a lane folds in place, 1 = none; lanes that own a value; values
    the last of them owns)."""
    chunk = 1
    while chunk * FOLD_LANES < items:
        chunk *= 2
    live = ceil_div(items, chunk)
    return chunk, live, items - (live - 1) * chunk


def pcg_live_columns(side):
    """Live lanes of a box's last column block (all 256 where side^2 is a multiple of 256)."""
    return side * side - COLUMNS * (ceil_div(side * side, COLUMNS) - 1)


def gram_plan(rows, cols, side):
    """gram_kernel: (pairs of the upper triangle, the most a lane owns, chunks a box is walked in, cells of the last chunk)."""
    assert 1 <= rows <= GRAM_MAX_SIDE and 1 <= cols <= GRAM_MAX_SIDE
    npairs = sum(max(cols - mm, 0) for mm in range(rows))
    chunks = ceil_div(side ** 3, GRAM_CHUNK)
    return npairs, ceil_div(npairs, GRAM_THREADS), chunks, side ** 3 - GRAM_CHUNK * (chunks - 1)


# ---------------------------------------------------------------------------------------------------------------------------- the passes alone
# geometry -> ((ncb, nseg, items), (chunk, live fold lanes, values of the last live lane)): the table of DESIGN.md §11.3 "The passes alone"
TABLE = {(1, 1): ((1, 1, 1), (1, 1, 1)),            # one live lane, six Dirichlet faces on one cell
         (1, 4): ((1, 1, 1), (1, 1, 1)),            # Solver's smallest box: 16 live columns
         (1, 12): ((1, 1, 1), (1, 1, 1)),           # one ragged segment of 12 planes
         (1, 20): ((2, 2, 4), (1, 4, 1)),           # a block starting mid-row, 144 live columns in the last, a second segment of 4 planes
         (3, 12): ((1, 1, 27), (1, 27, 1)),         # a box on no wall
         (2, 24): ((3, 2, 48), (1, 48, 1)),         # 64 live columns in the last block; a short last segment next to a neighbouring box
         (1, 40): ((7, 3, 21), (1, 21, 1)),         # three segments, the middle one full
         (1, 64): ((16, 4, 64), (1, 64, 1)),        # a power-of-two side
         (1, 104): ((43, 7, 301), (1, 301, 1)),     # rows longer than a wave that straddle blocks
         (15, 4): ((1, 1, 3375), (4, 844, 3)),      # the in-place fold: a ragged end inside a chunk
         (17, 4): ((1, 1, 4913), (8, 615, 1)),      # Solver(68, box_dim=4)
         (21, 4): ((1, 1, 9261), (16, 579, 13))}    # four in-place strides
PERIODIC = [(1, 12), (2, 24)]                       # a box that is its own neighbour; the wrap
ROWS = [(g, False) for g in TABLE] + [(g, True) for g in PERIODIC]
VARIANTS = {"7pt-cheby-helm": (1.3, 0.9), "7pt-cheby": (0.0, 0.9)}         # configuration -> (a, b) of the operator
VECTORS = 14
IDS = {"spare": H.VECTOR_TEMP, "x": H.VECTOR_U, "z": H.VECTOR_E, "r": H.VECTOR_R, "p": 12, "Ap": 13}
COEFFICIENTS = (H.VECTOR_ALPHA, H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
ALPHA_CG = 0.37


def row_id(row):
    return f"{row[0][0]}x{row[0][1]}" + ("-periodic" if row[1] else "")


def check_row(geom):
    """The row of TABLE against the plans above; returns (ncb, nseg, items)."""
    grid, plan = TABLE[geom]
    assert pcg_items(geom[1], geom[0] ** 3) == grid and pcg_fold_plan(grid[2]) == plan, (geom, pcg_items(geom[1], geom[0] ** 3), pcg_fold_plan(grid[2]))
    return grid


def new_level(be, geom, periodic=False):
    """A plain level of VECTORS vectors (the caller has configured a 7-point variant: one ghost cell)."""
    lv = be.level(geom[0], geom[1], num_vectors=VECTORS, bc=H.BC_PERIODIC if periodic else H.BC_DIRICHLET)
    assert (lv.num_vectors, lv.num_boxes, lv.box_dim, lv.ghosts) == (VECTORS, geom[0] ** 3, geom[1], 1)
    return lv


def coefficient_fields(oracle_level, seed):
    """alpha and the three betas in [0.5, 1.5), their box-to-box ghost copies exchanged on the oracle's level (face-centred data is shared by two
    boxes); the fields as that level then holds them, to be written to the level of the other side unchanged."""
    out = {}
    for n, vid in enumerate(COEFFICIENTS):
        oracle_level.write_all(vid, np.abs(random_field(oracle_level, seed + n)) + 0.5)
        oracle_level.b.lib.exchange_boundary(oracle_level.ptr, vid, H.STENCIL_SHAPE_BOX)
        out[vid] = oracle_level.read_all(vid)
    return out


def _scalar():
    return ctypes.c_double(-1.0)


def call_dot(lv, a, b):
    v = _scalar()
    return lv.b.lib.hpgmg_pcg_dot(lv.ptr, IDS.get(a, a), IDS.get(b, b), ctypes.byref(v)), v.value


def call_dot2(lv, a, c, b):
    v, w = _scalar(), _scalar()
    return lv.b.lib.hpgmg_pcg_dot2(lv.ptr, IDS.get(a, a), IDS.get(c, c), IDS.get(b, b), ctypes.byref(v), ctypes.byref(w)), v.value, w.value


def call_apply_dot(lv, Ap, p, a, b):
    v = _scalar()
    return lv.b.lib.hpgmg_pcg_apply_dot(lv.ptr, IDS.get(Ap, Ap), IDS.get(p, p), a, b, ctypes.byref(v)), v.value


def call_update(lv, x, r, p, Ap, alpha):
    v = _scalar()
    return lv.b.lib.hpgmg_pcg_update(lv.ptr, IDS.get(x, x), IDS.get(r, r), IDS.get(p, p), IDS.get(Ap, Ap), alpha, ctypes.byref(v)), v.value


def run_passes(lv, a, b):
    """apply_dot, update, dot, dot2 (and the dot of dot2's second pair) as an iteration issues them, on what the level holds.  Returns the return
    values ("took": 1 a kernel ran, 0 the portable form), the scalars, and the fields the passes wrote."""
    out, took = {}, {}
    took["apply_dot"], out["pAp"] = call_apply_dot(lv, "Ap", "p", a, b)
    out["Ap"], out["p"] = lv.read_all(IDS["Ap"]), lv.read_all(IDS["p"])
    took["update"], out["rmax"] = call_update(lv, "x", "r", "p", "Ap", ALPHA_CG)
    out["x"], out["r"] = lv.read_all(IDS["x"]), lv.read_all(IDS["r"])
    took["dot"], out["rz"] = call_dot(lv, "r", "z")
    took["dot2"], out["rz2"], out["Apz2"] = call_dot2(lv, "r", "Ap", "z")
    took["dot'"], out["Apz"] = call_dot(lv, "Ap", "z")
    out["took"] = took
    return out


def same_scalar(a, b):
    """Bit for bit; any NaN matches any NaN."""
    return (np.isnan(a) and np.isnan(b)) or bits(a).tolist() == bits(b).tolist()
