"""The s-step bottom solvers on the HIP path.

matmul() of the HIP plugin is one Gram launch (kernels/gram.hip); its matrix must equal the CPU oracle's matmul() -- the reference's order,
restated in tests/test_oracle_ca_bottom.py -- to the last bit, on every shape the solvers produce and on levels of many boxes.  `hpgmg-fv
--bottom-solver cabicgstab|cacg` must print the reference's lines (tests/golden/ca_bottom_norms.json), on one rank and on two processes
sharing the GPU."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from hpgmg_testlib import ROOT
from test_oracle_ca_bottom import CASES, GOLD, SHAPE_IDS, SHAPES, call_matmul, cli_args, parse, seeded_level, shape_vectors
import hpgmg_amd as H

pytestmark = pytest.mark.gpu
HIP_EXE = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def gram_on_both(hip, oracle, nb, d, g, id_A, id_B, nvec, seed):
    out = []
    for be in (hip, oracle):
        be.configure()
        lv = seeded_level(be, nb, d, g, nvec, seed)
        try:
            out.append(call_matmul(be.lib, lv, id_A, id_B))
        finally:
            lv.destroy()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_gram_launch_equals_the_oracle_matmul(hip, oracle, shape):
    nb, d, g, rows, cols, _ = shape
    nvec, id_A, id_B = shape_vectors(shape)
    got, want = gram_on_both(hip, oracle, nb, d, g, id_A, id_B, nvec, seed=11 + d)
    assert not np.isnan(got).any() and same_bits(got, want)
    assert len(set(want[:cols].tolist())) == len(set(id_B))        # the first row: one value per distinct vector of id_B, so a crossed slot shows


# bottom levels of many boxes (the U-cycle ladder keeps every box: 8 per side = 512 boxes of one or two cells), CABiCGStab's 17 x 18 and CACG's 9 x 9
@pytest.mark.parametrize("per_side", [1, 2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("d,g", [(1, 1), (2, 1), (2, 2), (4, 1)])
def test_gram_launch_per_box_count(hip, oracle, per_side, d, g):
    for rows, cols in ((17, 18), (9, 9)):
        got, want = gram_on_both(hip, oracle, per_side, d, g, list(range(rows)), list(range(cols)), cols, seed=100 * per_side + d)
        assert same_bits(got, want), (rows, cols)


def test_gram_launch_refuses_more_than_32_vectors_per_side():
    K = H.load_kernels()
    lvl = H.HipLevel()
    ids = (ctypes.c_int * 33)(*range(33))
    C = (ctypes.c_double * (33 * 33))()
    assert K.hpgmg_hip_gram(ctypes.byref(lvl), ids, 33, ids, 33, C) != 0      # refused before anything is launched


@pytest.mark.parametrize("case", CASES)
def test_hpgmg_fv_prints_the_reference_s_ca_lines(case):
    out = subprocess.run([HIP_EXE] + cli_args(case), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert parse(out.stdout) == GOLD[case]


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def run_ca_job(world, variant, log2, per_rank, solver, gather_dim, ucycles=0):
    """tests/test_multirank_gloo.py's run_job with the bottom solver chosen (tests/ca_multirank_worker.py)"""
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1", HPGMG_GATHER_DIM=str(gather_dim), HPGMG_GRAPH="1",
               HPGMG_TEST_BOTTOM_SOLVER=str(solver), HPGMG_TEST_UCYCLES=str(ucycles))
    cmd = ["timeout", "-k", "10", "500", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "ca_multirank_worker.py"), variant, str(log2), str(per_rank), "hip"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    dec, res, pos = json.JSONDecoder(), [], 0
    while True:
        pos = out.stdout.find("RESULT ", pos)
        if pos < 0:
            break
        obj, end = dec.raw_decode(out.stdout, pos + len("RESULT "))
        res.append(obj); pos = end
    assert len(res) == world
    return sorted(res, key=lambda r: r["rank"])


# the shapes tests/test_gpu_multirank.py pins with BiCGStab: two ranks x 4 boxes of 16^3 = the single-rank `4 8` domain; the reference's rank map (0) and
# the coarse levels gathered on rank 0 from 16^3 down (16)
@pytest.mark.parametrize("gather", [0, 16])
@pytest.mark.parametrize("variant", ["7pt-cheby-helm", "fv4-gsrb"])
@pytest.mark.parametrize("solver", ["cabicgstab", "cacg"])
def test_two_processes_print_the_single_rank_ca_numbers(solver, variant, gather):
    gold = GOLD[f"{solver} {variant} 4 8"]
    res = run_ca_job(2, variant, 4, 4, {"cabicgstab": H.BOTTOM_CABICGSTAB, "cacg": H.BOTTOM_CACG}[solver], gather)
    assert res[0]["norms"] == gold["norms"], res[0]
    assert res[0]["err"] == gold["richardson_error"] and res[0]["order"] == gold["order"]
    assert res[0]["repeat"] == [gold["norms"][0]] * 3, res[0]["repeat"]
    for r in res:      # every rank sees the reduced norms of the levels it is active on: h and 2h, or only h where 16^3 and below live on rank 0
        assert r["norms"][:2 if gather == 0 else 1] == gold["norms"][:2 if gather == 0 else 1], r
    for lv in range(1, len(res[0]["levels"])):
        if gather and res[0]["levels"][lv]["dim"] <= gather:
            assert res[0]["levels"][lv]["my_boxes"] > 0 and all(r["levels"][lv]["my_boxes"] == 0 for r in res[1:])


def test_two_processes_share_a_u_cycle_bottom_level():
    """U-cycles keep every box, so the bottom level of 8 boxes is split over the two ranks and matmul's one reduction of the whole matrix runs.  The
    ranks' partial matrices are added in rank order, which associates the box sums differently from one rank: equal to the fixture to 1e-9."""
    gold = GOLD["cabicgstab 7pt-cheby-ucycle 4 8"]
    res = run_ca_job(2, "7pt-cheby", 4, 4, H.BOTTOM_CABICGSTAB, 0, ucycles=1)
    assert res[0]["levels"][-1]["my_boxes"] == 4 and res[1]["levels"][-1]["my_boxes"] == 4
    for r in res:
        assert np.allclose([float(x) for x in r["norms"]], [float(x) for x in gold["norms"]], rtol=1e-9, atol=0), r["norms"]
