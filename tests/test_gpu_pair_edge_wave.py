"""The EDGEW instances of the sweep-pair kernel (kernels/cheby_pair.hpp): where a row has more than one 128-cell tile, an eleventh wave of the workgroup forms x1 on the
two cell columns next to the tile and hands them -- and x0 of the same columns -- to lanes 0 / 63 of the ten main waves through LDS; the launch has no pre-pass
(cheby_pair_edge_kernel) and x1 of those columns never goes through memory.  The arithmetic per cell is the pre-pass's, so nothing about the result may change: VECTOR_U and
VECTOR_TEMP after smooth() are the oracle's bytes whatever the chunk length, and the same bytes come from the pre-pass path, which every launch outside the first cut keeps
(HPGMG_TUNE_PAIR_PACKED=0: no packed coefficient values; HPGMG_TUNE_PAIR_NW=12: a wave count without EDGEW instances; GSRB).  hpgmg_hip_pair_edge_wave_launches() says
which path ran.

The geometry is 256^3 in 2^3 boxes of 128, the smallest level with an interior tile edge: slabs at both j walls, chunks at both k walls and both sides of the tile edge are
inside it.  The knobs are read once per process, so every setting runs in a worker process: this file run as a script does the cases named in PAIR_EDGEW_CASES and prints
one JSON line each.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (the OpenMP environment of the suite, before any runtime loads)

import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, Backend, load_golden
from test_gpu_operators import make_pair

pytestmark = pytest.mark.gpu

GEOM = (2, 128)
CASES = {"helm": "7pt-cheby-helm", "cheby": "7pt-cheby", "gsrb": "7pt-gsrb"}
CHEBY = ["helm", "cheby"]
OUT = (H.VECTOR_U, H.VECTOR_TEMP)
KNOBS = ("HPGMG_TUNE_PAIR_NW", "HPGMG_TUNE_PAIR_KC", "HPGMG_TUNE_PAIR_PACKED")
# 10 waves and a chunk length (0 = the launcher's choice, 64 here).  KC 1: every step is general; 2 / 3: the shortest segments; 24: the chunk 120..143 crosses the box
# face at 128; 50: a short last chunk of 6 planes
EDGEW_SHAPES = [(10, 0), (10, 1), (10, 2), (10, 3), (10, 24), (10, 50)]
PREPASS = {"packed-0": {"HPGMG_TUNE_PAIR_PACKED": "0"}, "nw-12": {"HPGMG_TUNE_PAIR_NW": "12"}}


def shape_env(nw, kc):
    env = {"HPGMG_TUNE_PAIR_NW": str(nw)}
    if kc:
        env["HPGMG_TUNE_PAIR_KC"] = str(kc)
    return env


def smooth_case(hip, oracle, variant):
    K = H.load_kernels()
    K.hpgmg_hip_pair_edge_wave_launches.restype = ctypes.c_longlong
    lh, lo = make_pair(hip, oracle, variant, *GEOM, seed=7)
    try:
        a, b = (1.0, 1.0) if "helm" in variant else (0.0, 1.0)
        res, launches, edge_wave = [], (ctypes.c_longlong * 2)(), []
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, a, b)
            K.hpgmg_hip_pair_launch_counts(launches)
            before = (int(launches[0]), int(K.hpgmg_hip_pair_edge_wave_launches()))
            lv.b.lib.smooth(lv.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
            res.append([lv.interior(v) for v in OUT])            # (reading a vector issues a postponed smooth())
            K.hpgmg_hip_pair_launch_counts(launches)
            edge_wave.append((int(launches[0]) - before[0], int(K.hpgmg_hip_pair_edge_wave_launches()) - before[1]))
        got, ref = res
        return {"is_oracle": all(np.array_equal(x, y) for x, y in zip(got, ref)), "sha": hashlib.sha256(b"".join(x.tobytes() for x in got)).hexdigest(),
                "pair_launches": edge_wave[0][0], "edge_wave_launches": edge_wave[0][1], "oracle_side_launches": edge_wave[1][0]}
    finally:
        lh.destroy(); lo.destroy()


def worker():
    hip, oracle = Backend.hip(), Backend.oracle()
    hip.lib.hpgmg_set_pair_min_cells.argtypes = [ctypes.c_longlong]
    hip.lib.hpgmg_set_pair_min_cells(1 << 20)
    for name in os.environ["PAIR_EDGEW_CASES"].split(","):
        print("CASE " + json.dumps(dict(smooth_case(hip, oracle, CASES[name]), case=name)), flush=True)


_RUNS = {}


def run_with(knobs, names):
    key = tuple(sorted(knobs.items()))
    if key not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(knobs, PAIR_EDGEW_CASES=",".join(names))
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
        rows = [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CASE ")]
        _RUNS[key] = {r["case"]: r for r in rows}
        assert sorted(_RUNS[key]) == sorted(names)
    return _RUNS[key]


def first_run():
    """10 waves, the launcher's chunk length; the one worker that also does the GSRB case."""
    return run_with(shape_env(*EDGEW_SHAPES[0]), CHEBY + ["gsrb"])


@pytest.mark.parametrize("nw,kc", EDGEW_SHAPES)
@pytest.mark.parametrize("case", CHEBY)
def test_the_edge_wave_gives_the_oracles_bits_at_every_chunk_length(case, nw, kc):
    """smooth() through the EDGEW instances: both outputs are the oracle's bytes, one digest for every chunk length, and every pair launch was an edge-wave launch."""
    r = (first_run() if (nw, kc) == EDGEW_SHAPES[0] else run_with(shape_env(nw, kc), CHEBY))[case]
    print(case, nw, kc, r)
    assert r["is_oracle"]
    assert r["sha"] == first_run()[case]["sha"]
    assert r["pair_launches"] >= 2 and r["edge_wave_launches"] >= 2
    assert r["edge_wave_launches"] == r["pair_launches"]
    assert r["oracle_side_launches"] == 0


@pytest.mark.parametrize("path", list(PREPASS))
@pytest.mark.parametrize("case", CHEBY)
def test_the_pre_pass_path_gives_the_same_bits(case, path):
    """Without the packed coefficient values, or with 12 waves, the launch keeps its pre-pass: the same digest, and no edge-wave launch."""
    r = run_with(PREPASS[path], CHEBY)[case]
    print(case, path, r)
    assert r["is_oracle"]
    assert r["sha"] == first_run()[case]["sha"]
    assert r["pair_launches"] >= 2 and r["edge_wave_launches"] == 0


def test_gsrb_keeps_the_pre_pass():
    """GSRB half-sweep pairs at the same geometry have no EDGEW instance: the oracle's bytes by the pre-pass path."""
    r = first_run()["gsrb"]
    print(r)
    assert r["is_oracle"]
    assert r["pair_launches"] >= 1 and r["edge_wave_launches"] == 0


_CYCLE = {}


def cycle_lines(packed):
    from test_gpu_parity_sweep import pinned_lines
    if packed not in _CYCLE:
        exe = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")
        _CYCLE[packed] = pinned_lines(exe, "--helmholtz", "7 8", **({} if packed else {"HPGMG_TUNE_PAIR_PACKED": "0"}))
    return _CYCLE[packed]


def test_the_whole_cycle_prints_the_same_lines_on_either_path():
    """hpgmg-fv --helmholtz 7 8 (256^3 in boxes of 128): the up-leg's smooth() on the fine level takes the INTERP instance of the edge wave, whose x0 carries the coarse
    parent.  The pinned lines are those of the pre-pass path, and the F-cycle norms the reference's."""
    lines = cycle_lines(True)
    assert len(lines) >= 10 and lines == cycle_lines(False)
    gold = load_golden("fcycle_norms.json")["7pt-cheby-helm 7 8"]
    printed = [re.search(r"norm=(\S+)", l).group(1) for l in lines if "f-cycle" in l]
    assert [g for g in gold["norms"] if g in printed] == gold["norms"], (gold["norms"], printed[:6])


if __name__ == "__main__":
    worker()
