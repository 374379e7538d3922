"""The reference's s-step bottom solvers (-DUSE_CABICGSTAB: solvers/cabicgstab.c, -DUSE_CACG: solvers/cacg.c) on the CPU oracle.

`hpgmg-fv-oracle --bottom-solver cabicgstab|cacg` must print the lines the reference prints when built with those flags (recorded in
tests/golden/ca_bottom_norms.json), and the oracle's matmul() -- host/solvers.c's weak default -- must follow the reference's summation order:
per box one chain over the interior in k, j, i order, box partials added in box order (not dot()'s per-tile order)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hpgmg_testlib import ROOT, Backend, build_oracle, load_golden, seeded_field
import hpgmg_amd as H
from pcg_lib import gram_plan, gram_restated

GOLD = load_golden("ca_bottom_norms.json")
SOLVERS = {"cabicgstab": H.BOTTOM_CABICGSTAB, "cacg": H.BOTTOM_CACG}
FLAGS = {"7pt-cheby": [], "7pt-cheby-helm": ["--helmholtz"], "27pt-gsrb": ["--op", "27pt", "--smoother", "gsrb"], "fv4-gsrb": ["--op", "fv4", "--smoother", "gsrb"],
         "7pt-cheby-ucycle": ["--ucycles"], "fv4-gsrb-ucycle": ["--ucycles", "--op", "fv4", "--smoother", "gsrb"]}
CASES = sorted(k for k in GOLD if not k.startswith("_"))


def parse(out):
    """the fields tests/golden/ca_bottom_norms.json holds, from one run's output"""
    fc = re.findall(r"f-cycle\s+norm=(\S+)\s+rel=(\S+)", out)[-3:]
    return {"norms": [n for n, _ in fc], "rels": [r for _, r in fc], "richardson_error": re.search(r"\|\|error\|\|=(\S+)", out).group(1),
            "order": re.search(r"order=(\S+)", out).group(1), "eigenvalue_max": re.findall(r"eigenvalue_max<(\S+)", out),
            "lambda_max": re.findall(r"lambda_max\.\.\. <(\S+)", out),
            "levels": [[int(a), int(b), int(c)] for a, b, c in re.findall(r"attempting to create a (\d+)\^3 level from (\d+) x (\d+)\^3 boxes", out)]}


def cli_args(case):
    solver, variant, args = case.split(" ", 2)
    return ["--bottom-solver", solver] + FLAGS[variant] + ["--warmup", "0", "--solves", "1"] + args.split()


def test_fixture_covers_every_case_for_both_solvers():
    for solver in SOLVERS:
        for want in ("7pt-cheby 4 8", "7pt-cheby 4 27", "7pt-cheby 5 8", "7pt-cheby-helm 4 27", "27pt-gsrb 4 27", "fv4-gsrb 4 27", "7pt-cheby-ucycle 5 8"):
            assert f"{solver} {want}" in GOLD
    # the cases tell the solvers apart: `4 8` CA from BiCGStab, `4 27` CACG from CABiCGStab
    assert GOLD["cabicgstab 7pt-cheby 4 8"]["norms"][0] != load_golden("fcycle_norms.json")["7pt-cheby 4 8"]["norms"][0]
    assert GOLD["cabicgstab 7pt-cheby 4 27"]["norms"][0] != GOLD["cacg 7pt-cheby 4 27"]["norms"][0]


@pytest.mark.parametrize("case", CASES)
def test_oracle_prints_the_reference_s_ca_lines(case):
    build_oracle()
    out = subprocess.run([os.path.join(ROOT, "oracle", "hpgmg-fv-oracle")] + cli_args(case), capture_output=True, text=True,
                         env=dict(os.environ, OMP_NUM_THREADS="1"), check=True, timeout=600).stdout
    assert parse(out) == GOLD[case]


def test_bottom_solver_setter_round_trips_and_unknown_values_select_bicgstab():
    lib = Backend.oracle().lib
    try:
        for v in (H.BOTTOM_BICGSTAB, H.BOTTOM_CG, H.BOTTOM_CABICGSTAB, H.BOTTOM_CACG):
            lib.hpgmg_set_bottom_solver(v)
            assert lib.hpgmg_get_bottom_solver() == v
        for v in (-1, 4, 99):
            lib.hpgmg_set_bottom_solver(v)
            assert lib.hpgmg_get_bottom_solver() == H.BOTTOM_BICGSTAB
    finally:
        lib.hpgmg_set_bottom_solver(H.BOTTOM_BICGSTAB)


def test_cli_rejects_an_unknown_bottom_solver():
    build_oracle()
    out = subprocess.run([os.path.join(ROOT, "oracle", "hpgmg-fv-oracle"), "--bottom-solver", "gmres", "4", "8"], capture_output=True, text=True, timeout=60)
    assert "cabicgstab|cacg" in out.stderr and "f-cycle" not in out.stdout


# ---- matmul(): the order contract, restated in NumPy -------------------------------------------------------------------------------------------
def interiors(level, vid):
    """per box, the interior of vector vid as a flat k, j, i array"""
    d, g = level.box_dim, level.ghosts
    return [level.read(b, vid)[g:g + d, g:g + d, g:g + d].reshape(-1) for b in range(level.num_boxes)]


def numpy_matmul(level, id_A, id_B):
    rows, cols = len(id_A), len(id_B)
    C = np.zeros(rows * cols)
    A = {v: interiors(level, v) for v in set(id_A) | set(id_B)}
    for mm in range(rows):
        for nn in range(mm, cols):
            total = 0.0
            for b in range(level.num_boxes):
                chain = np.cumsum(A[id_A[mm]][b] * A[id_B[nn]][b])      # np.cumsum is sequential: the chain in k, j, i order
                total = total + float(chain[-1])                      # boxes in box order
            C[mm * cols + nn] = total
            if mm < cols and nn < rows:
                C[nn * cols + mm] = total
    return C


def call_matmul(lib, level, id_A, id_B):
    rows, cols = len(id_A), len(id_B)
    C = (ctypes.c_double * (rows * cols))(*([np.nan] * (rows * cols)))
    lib.matmul(level.ptr, C, (ctypes.c_int * rows)(*id_A), (ctypes.c_int * cols)(*id_B), rows, cols, 1)
    return np.array(C[:])


def seeded_level(backend, boxes_in_i, box_dim, ghosts, nvec, seed):
    lv = backend.level(boxes_in_i, box_dim, ghosts=ghosts, num_vectors=nvec)
    for v in range(nvec):
        lv.write_all(v, seeded_field(lv, seed + 7 * v))
    return lv


# (boxes per side, box side, ghosts, rows, cols, ids): ids True = id_A a prefix of id_B = 0 .. cols - 1, False = two scattered lists, or (id_A, id_B)
SHAPES = [(1, 3, 1, 17, 18, True),      # CABiCGStab at s = 4 on a 3^3 bottom box: 17 x 18, mirrored
          (1, 3, 2, 9, 9, True),        # CACG at s = 4, ghosts 2 (fv4)
          (2, 2, 2, 17, 18, True),      # eight boxes of 2^3 (fv4 U-cycle bottom)
          (3, 1, 1, 5, 6, True),        # 27 boxes of one cell, s = 1
          (2, 16, 1, 17, 18, True),     # boxes of several dim x 8 x 8 tiles: dot()'s order differs here
          (1, 24, 2, 9, 9, True),
          (2, 4, 1, 7, 3, False),       # id_A != id_B, rows > cols
          (2, 8, 1, 4, 11, False),
          # the edges of the launch (kernels/gram.hip; the plans of pcg_lib.gram_plan in GRAM_PLANS below)
          (2, 4, 1, 32, 32, True),      # 528 pairs: three per lane, the third slot live in lanes 0 - 15 only
          (1, 5, 1, 23, 23, True),      # 276 pairs: the second slot live in 20 lanes; 125 cells = one full chunk + 61
          (1, 6, 1, 32, 32, (list(range(32)), list(range(32, 64)))),      # 64 staged vectors, the full 33 KB of LDS; 216 = 3 * 64 + 24
          (1, 7, 2, 5, 3, ([0, 1, 0, 2, 1], [3, 0, 3])),                  # repeated ids on both sides; ghosts 2; rows > cols
          (1, 13, 1, 20, 5, (list(range(20)), list(range(5)))),           # rows > 16 > cols; 2197 = 34 * 64 + 21; rows >= cols stay as matmul leaves them
          (3, 5, 1, 17, 18, True)]      # the product's shape on 27 ragged boxes: a box-order sum of ragged chains
# rows, cols, side -> (pairs, most pairs of a lane, chunks, cells of the last chunk)
GRAM_PLANS = {(32, 32, 4): (528, 3, 1, 64), (23, 23, 5): (276, 2, 2, 61), (32, 32, 6): (528, 3, 4, 24), (5, 3, 7): (6, 1, 6, 23),
              (20, 5, 13): (15, 1, 35, 21), (17, 18, 5): (170, 1, 2, 61)}
SHAPE_IDS = [f"{s[0]}x{s[1]}g{s[2]}-{s[3]}x{s[4]}" for s in SHAPES]


def shape_vectors(shape):
    """(vectors of the level, id_A, id_B) of a shape; asserts its plan where GRAM_PLANS names one"""
    nb, d, g, rows, cols, ids = shape
    if ids is True:
        nvec, id_A, id_B = max(rows, cols), list(range(rows)), list(range(cols))
    elif ids is False:
        nvec = max(rows, cols) + rows + 2
        id_A, id_B = [nvec - 1 - m for m in range(rows)], [(3 * n + 1) % nvec for n in range(cols)]
    else:
        id_A, id_B = ids
        nvec = max(id_A + id_B) + 1
    assert (len(id_A), len(id_B)) == (rows, cols)
    if (rows, cols, d) in GRAM_PLANS:
        assert gram_plan(rows, cols, d) == GRAM_PLANS[rows, cols, d]
    return nvec, id_A, id_B


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_oracle_matmul_follows_the_reference_order(shape):
    nb, d, g, rows, cols, _ = shape
    be = Backend.oracle()
    be.configure()
    nvec, id_A, id_B = shape_vectors(shape)
    lv = seeded_level(be, nb, d, g, nvec, seed=11 + d)
    try:
        got = call_matmul(be.lib, lv, id_A, id_B)
        want = numpy_matmul(lv, id_A, id_B)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert np.array_equal(got.view(np.uint64), gram_restated(lv, id_A, id_B).view(np.uint64))        # the chain as a Python loop
        if d >= 16:     # more than one tile per box: the per-tile order of dot() gives other bits, so matmul cannot be built from dot()
            dots = [be.lib.dot(lv.ptr, id_A[0], id_B[n]) for n in range(cols)]
            assert any(dots[n] != got[n] for n in range(cols))
    finally:
        lv.destroy()
