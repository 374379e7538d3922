"""What the tests of the block hooks (include/hpgmg_operators.h hpgmg_block_gram / _combine / _residual; kernels/block.hip) share:
NumPy restatements of the three order contracts, the rows of pcg_lib.TABLE that exercise the mapping, the list sizes at the edges of the pair tile, and
the cases as data, so that tests/test_oracle_block_hooks.py (the portable forms against the restatements) and tests/test_gpu_block_hooks.py (the
kernels against both) run the same calls.

A level here is a plain one of `vectors_of(geom)` vectors.  Vector 0 is the weight (in [0.5, 1.5)); the others hold values in [-1, 1).  Every ghost and
padding double of every vector is NaN: a result that read one is not finite, and an output whose ghost or padding changed shows as other bits.
"""
import ctypes

import numpy as np

import hpgmg_amd as H
import pcg_lib as P
from reduction_lib import bits, cell_offsets, random_field

TILE = 6                                      # HPGMG_HIP_BLOCK_TILE: a lane carries TILE x TILE pair chains
MAX_IN, MAX_OUT = H.BLOCK_MAX_IN, H.BLOCK_MAX_OUT
SIZES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, MAX_IN]
# (boxes per side, box side): one partial column block, ragged segments, a block starting mid-row, many boxes in the fold, the in-place fold strides
ROWS = [(1, 4), (1, 12), (1, 20), (3, 12), (2, 24), (1, 40), (17, 4)]
W_ID = 0
_c_int_p, _c_dbl_p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)


def row_id(geom):
    return f"{geom[0]}x{geom[1]}"


def vectors_of(geom):
    """4913 boxes hold fewer vectors (and their lists stop at TILE + 1: the fold over many workgroup values is what the row is for)."""
    return 16 if geom == (17, 4) else 48


def sizes_of(geom):
    return [s for s in SIZES if s <= (TILE + 1 if geom == (17, 4) else MAX_IN)]


def new_level(be, geom):
    lv = be.level(geom[0], geom[1], num_vectors=vectors_of(geom))
    assert (lv.num_vectors, lv.num_boxes, lv.box_dim, lv.ghosts) == (vectors_of(geom), geom[0] ** 3, geom[1], 1)
    return lv


def nan_outside(level, field):
    out = np.full_like(field, np.nan)
    q = cell_offsets(level)
    out[:, q] = field[:, q]
    return out


def fields_of(level, seed):
    """vector id -> field: random interiors, NaN everywhere else; the weight positive."""
    F = {v: nan_outside(level, random_field(level, seed + v)) for v in range(level.num_vectors)}
    F[W_ID] = np.abs(F[W_ID]) + 0.5
    return F


def write_fields(lv, F, ids=None):
    for v in (F if ids is None else ids):
        lv.write_all(v, F[v])


def _ids(ids):
    return (ctypes.c_int * len(ids))(*ids)


# ---------------------------------------------------------------------------------------------------------------------------- the calls
def call_gram(lv, a, b, w, host=False):
    G = np.full(len(a) * len(b), np.nan)
    fn = lv.b.lib.hpgmg_block_gram_host if host else lv.b.lib.hpgmg_block_gram
    return fn(lv.ptr, _ids(a), len(a), _ids(b), len(b), w, G.ctypes.data_as(_c_dbl_p)), G.reshape(len(a), len(b))


def call_combine(lv, out_ids, in_ids, C, host=False):
    C = np.ascontiguousarray(C, dtype=np.float64)
    assert C.shape == (len(in_ids), len(out_ids))
    fn = lv.b.lib.hpgmg_block_combine_host if host else lv.b.lib.hpgmg_block_combine
    return fn(lv.ptr, _ids(out_ids), len(out_ids), _ids(in_ids), len(in_ids), C.ctypes.data_as(_c_dbl_p))


def call_residual(lv, r_ids, ax_ids, x_ids, w, mu, host=False):
    n = len(r_ids)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    rmax, mxmax = np.full(n, np.nan), np.full(n, np.nan)
    fn = lv.b.lib.hpgmg_block_residual_host if host else lv.b.lib.hpgmg_block_residual
    rc = fn(lv.ptr, _ids(r_ids), _ids(ax_ids), _ids(x_ids), n, w, mu.ctypes.data_as(_c_dbl_p), rmax.ctypes.data_as(_c_dbl_p), mxmax.ctypes.data_as(_c_dbl_p))
    return rc, rmax, mxmax


# ---------------------------------------------------------------------------------------------------------------------------- the contracts, restated
def gram_restated(level, F, a, b, w):
    """Entry (i, j): ONE tree of the CG passes' order (pcg_lib.header_order_dot) over the leaf terms a_i * b_j, weighted (w * a_i) * b_j in that
    association; identical lists: the lower triangle is a copy of the upper."""
    q = cell_offsets(level)
    I = {v: F[v][:, q] for v in set(a) | set(b)}
    wa = {v: (F[w][:, q] * I[v] if w >= 0 else I[v]) for v in set(a)}
    same = list(a) == list(b)
    G = np.empty((len(a), len(b)))
    for i, va in enumerate(a):
        for j, vb in enumerate(b):
            G[i, j] = G[j, i] if same and j < i else P.header_order_dot(wa[va], I[vb], level.box_dim)
    return G


def combine_restated(level, F, out_ids, in_ids, C):
    """out_j = sum_i C[i, j] in_i per interior cell: the chain starts at 0.0, runs i = 0 .. nin - 1, each product formed first; every input is the
    vector as it was BEFORE the call.  Returns {output id: field}; ghost and padding doubles keep what F holds."""
    q = cell_offsets(level)
    out = {}
    for j, vo in enumerate(out_ids):
        acc = np.zeros(F[vo][:, q].shape)
        for i, vi in enumerate(in_ids):
            acc = acc + C[i, j] * F[vi][:, q]
        out[vo] = F[vo].copy()
        out[vo][:, q] = acc
    return out


def residual_restated(level, F, r_ids, ax_ids, x_ids, w, mu):
    """r_j = ax_j - mu_j * (w * x_j), the product w * x first; max |r_j| and max |w x_j| from 0.0, a NaN never the maximum.  Returns ({r id: field},
    rmax, mxmax)."""
    q = cell_offsets(level)
    out, rmax, mxmax = {}, [], []
    for j, (vr, va, vx) in enumerate(zip(r_ids, ax_ids, x_ids)):
        mx = F[w][:, q] * F[vx][:, q] if w >= 0 else F[vx][:, q]
        r = F[va][:, q] - mu[j] * mx
        out[vr] = F[vr].copy()
        out[vr][:, q] = r
        rmax.append(float(np.fmax.reduce(np.abs(r).ravel(), initial=0.0)))
        mxmax.append(float(np.fmax.reduce(np.abs(mx).ravel(), initial=0.0)))
    return out, np.array(rmax), np.array(mxmax)


# ---------------------------------------------------------------------------------------------------------------------------- the cases
def gram_cases(geom):
    """name -> (a ids, b ids): identical lists of every size, na != nb, an id in both lists, 1 x 1, and the widest requests."""
    pool = list(range(1, vectors_of(geom)))
    cases = {f"identical-{s}": (pool[:s], pool[:s]) for s in sizes_of(geom)}
    cases["1x1"] = (pool[:1], pool[1:2])
    cases[f"{TILE + 1}x{TILE - 1}"] = (pool[:TILE + 1], pool[-(TILE - 1):])
    cases[f"{TILE - 1}x{TILE + 1}-overlap"] = (pool[:TILE - 1], pool[2:TILE + 3])
    if MAX_IN in sizes_of(geom):
        cases[f"{MAX_IN}x1"] = (pool[:MAX_IN], pool[40:41])
        cases[f"{2 * TILE + 1}x{MAX_IN}-overlap"] = (pool[:2 * TILE + 1], pool[5:5 + MAX_IN])
        cases[f"{TILE}x{2 * TILE + 1}"] = (pool[20:20 + TILE], pool[:2 * TILE + 1])
    return cases


def combine_cases(geom):
    """name -> (out ids, in ids, zero column or None).  "alias": the outputs are the first inputs (X both read and written)."""
    pool = list(range(1, vectors_of(geom)))
    wide = min(MAX_IN, len(pool))
    cases = {"1-to-1": (pool[-1:], pool[:1], None),
             "alias-7-to-5": (pool[:5], pool[:7], None),
             "alias-wide-to-12": (pool[:MAX_OUT], pool[:wide], 3),
             "1-to-12": (pool[1:1 + MAX_OUT], pool[:1], None),
             "wide-to-1-alias-last": (pool[wide - 1:wide], pool[:wide], None)}
    if geom == (17, 4):                       # 4913 boxes: the row is there for the folds; the combination meets nothing new on it
        cases = {name: cases[name] for name in ("1-to-1", "alias-7-to-5")}
    if len(pool) >= MAX_IN + MAX_OUT - 1:
        cases["36-to-12-disjoint"] = ([W_ID] + pool[MAX_IN:MAX_IN + MAX_OUT - 1], pool[:MAX_IN], 0)
    return cases


def combine_matrix(nin, nout, zero_column, seed):
    C = np.random.default_rng(seed).random((nin, nout)) * 2.0 - 1.0
    if zero_column is not None:
        C[:, zero_column] = 0.0
    return C


def residual_cases(geom):
    """name -> (r ids, ax ids, x ids)"""
    pool = list(range(1, vectors_of(geom)))
    n = min(MAX_OUT, len(pool) // 3)
    return {"1": (pool[2:3], pool[0:1], pool[1:2]), f"{n}": (pool[2 * n:3 * n], pool[:n], pool[n:2 * n])}


def last_live_cell(level):
    """(box, raw offset) of the cell the last live lane of the last workgroup meets last: the last column of the last box, its last plane."""
    d = level.box_dim
    return level.num_boxes - 1, int(cell_offsets(level)[d - 1, d - 1, d - 1])


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: other bits at {bad[:5].tolist()} ..."
