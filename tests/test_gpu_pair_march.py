"""The k-march of the sweep-pair kernel runs in segments (kernels/cheby_pair.hpp): inside one box, away from the ends of the chunk and of the domain, a step takes its
addresses from the segment and tests nothing about the plane; the first step, the steps next to a box face and the last ones take the general form.  Where one form hands
over to the other depends on the chunk length KC, the box size and the position of the chunk, not on the result: whatever the shape, VECTOR_U and VECTOR_TEMP after
smooth() are the oracle's, byte for byte, and so the same for every shape.

HPGMG_TUNE_PAIR_NW and HPGMG_TUNE_PAIR_KC are read once per process, so every shape runs in a worker process: this file run as a script does the cases named in
PAIR_MARCH_CASES and prints one JSON line each.
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

# name -> variant, (boxes per side, box side).  128^3 is the smallest level the kernel takes (a row is 128 cells).  One box: no box face inside a march.  2^3 boxes of 64: the
# NARROW instances, a box face at plane 64.  2^3 boxes of 128 (256^3): an interior tile edge in i, lanes 0 / 63 read their neighbour columns.
SMALL = {
    "helm-1x128": ("7pt-cheby-helm", (1, 128)), "cheby-1x128": ("7pt-cheby", (1, 128)), "gsrb-1x128": ("7pt-gsrb", (1, 128)),
    "helm-2x64": ("7pt-cheby-helm", (2, 64)), "cheby-2x64": ("7pt-cheby", (2, 64)), "gsrb-2x64": ("7pt-gsrb", (2, 64)),
}
EDGE = {"helm-2x128": ("7pt-cheby-helm", (2, 128))}
CASES = dict(SMALL, **EDGE)
OUT = (H.VECTOR_U, H.VECTOR_TEMP)
# (waves, KC) -- 0 = the launcher's choice.  With 10 waves, KC = 1: no step qualifies for a segment; 2: the shortest segment, one step; 3: two steps;
# 8: what the launcher picks at 128^3; 24: the chunk 48..71 crosses the box face at 64 of the second geometry after a segment has begun; 50: a short last chunk (28 planes);
# 64: chunks end at the box face; 128: one chunk per column, two segments in the second geometry.
SHAPES_SMALL = [(10, kc) for kc in (1, 2, 3, 8, 24, 50, 64, 128)] + [(nw, kc) for nw in (12, 16) for kc in (1, 24)]
SHAPES_EDGE = [(0, 0), (0, 24)]


def coefficients_of(variant):
    return (1.0, 1.0) if "helm" in variant else (0.0, 1.0)


def smooth_case(hip, oracle, variant, geom):
    lh, lo = make_pair(hip, oracle, variant, *geom, seed=7)
    try:
        a, b = coefficients_of(variant)
        res = []
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, a, b)
            lv.b.lib.smooth(lv.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
            res.append([lv.interior(v) for v in OUT])
        got, ref = res
        launches = (ctypes.c_longlong * 2)()
        H.load_kernels().hpgmg_hip_pair_launch_counts(launches)
        return {"is_oracle": all(np.array_equal(x, y) for x, y in zip(got, ref)), "sha": hashlib.sha256(b"".join(x.tobytes() for x in got)).hexdigest(),
                "pair_launches": int(launches[0])}
    finally:
        lh.destroy(); lo.destroy()


def worker():
    hip, oracle = Backend.hip(), Backend.oracle()
    hip.lib.hpgmg_set_pair_min_cells.argtypes = [ctypes.c_longlong]
    hip.lib.hpgmg_set_pair_min_cells(1 << 20)
    for name in os.environ["PAIR_MARCH_CASES"].split(","):
        variant, geom = CASES[name]
        print("CASE " + json.dumps(dict(smooth_case(hip, oracle, variant, geom), case=name)), flush=True)


_RUNS, _STDERR = {}, {}


def run_with(nw, kc, names):
    if (nw, kc) not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k not in ("HPGMG_TUNE_PAIR_NW", "HPGMG_TUNE_PAIR_KC")}
        env["PAIR_MARCH_CASES"] = ",".join(names)
        if nw:
            env["HPGMG_TUNE_PAIR_NW"] = str(nw)
        if kc:
            env["HPGMG_TUNE_PAIR_KC"] = str(kc)
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
        rows = [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CASE ")]
        _RUNS[(nw, kc)] = {r["case"]: r for r in rows}
        _STDERR[(nw, kc)] = out.stderr
        assert sorted(_RUNS[(nw, kc)]) == sorted(names)
    return _RUNS[(nw, kc)]


def check(case, nw, kc, names, first_shape):
    r = run_with(nw, kc, names)[case]
    print(case, nw, kc, r)
    assert r["is_oracle"]
    assert r["sha"] == run_with(*first_shape, names)[case]["sha"]


@pytest.mark.parametrize("nw,kc", SHAPES_SMALL)
@pytest.mark.parametrize("case", list(SMALL))
def test_every_chunk_length_gives_the_oracles_bits(case, nw, kc):
    """Both outputs of smooth() equal the oracle's, and their digest is the same for every (waves, KC)."""
    check(case, nw, kc, list(SMALL), SHAPES_SMALL[0])
    # the pair kernel ran (two launches per smooth(), more as the worker goes through its cases): a level it refused would be smoothed by the single-sweep kernels
    assert run_with(nw, kc, list(SMALL))[case]["pair_launches"] >= 2


def test_a_refused_wave_count_is_the_launchers_choice():
    """HPGMG_TUNE_PAIR_NW=11 names no instance of the kernel.  The launcher reads the knob table (kernels/knobs.hip), not the variable: the table refuses 11 with one line
    on stderr and gives 0, the cost model's choice -- the oracle's bits, the digest of every other shape, and the pair kernel ran."""
    case = list(SMALL)[0]
    r = run_with(11, 0, [case])[case]
    print(case, 11, 0, r)
    assert r["is_oracle"]
    assert r["sha"] == run_with(*SHAPES_SMALL[0], list(SMALL))[case]["sha"]
    assert r["pair_launches"] >= 2
    refusals = [l for l in _STDERR[(11, 0)].splitlines() if l.startswith("hpgmg_hip: HPGMG_TUNE_PAIR_NW=11 is not accepted")]
    assert len(refusals) == 1 and refusals[0].endswith("using 0"), _STDERR[(11, 0)][-800:]


@pytest.mark.parametrize("nw,kc", SHAPES_EDGE)
def test_tile_edge_columns(nw, kc):
    """256^3 in boxes of 128: two tiles per row, so lanes 0 and 63 read x0 and the pre-pass's x1 across the tile edge -- from segment bases in the steady steps."""
    check("helm-2x128", nw, kc, list(EDGE), SHAPES_EDGE[0])
    assert run_with(nw, kc, list(EDGE))["helm-2x128"]["pair_launches"] >= 2


_FOLD = {}


def fold_lines(size, kc):
    from test_gpu_parity_sweep import pinned_lines
    if (size, kc) not in _FOLD:
        exe = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")
        _FOLD[(size, kc)] = pinned_lines(exe, "--helmholtz", size, **({"HPGMG_TUNE_PAIR_KC": str(kc)} if kc else {}))
    return _FOLD[(size, kc)]


@pytest.mark.parametrize("size,kc", [("6 8", 0), ("6 8", 3), ("6 8", 24), ("7 1", 24)])
def test_the_fold_prints_the_same_lines_at_every_chunk_length(size, kc):
    """hpgmg-fv --helmholtz with a fine level of 128^3 (6 8: boxes of 64; 7 1: one box): the up-leg's smooth() takes the INTERP instances, whose segments also carry
    the addresses of the coarse parents."""
    lines = fold_lines(size, kc)
    assert len(lines) >= 10 and lines == fold_lines(size, 0)
    gold = load_golden("fcycle_norms.json").get("7pt-cheby-helm " + size)
    if gold:
        printed = [re.search(r"norm=(\S+)", l).group(1) for l in lines if "f-cycle" in l]
        assert [g for g in gold["norms"] if g in printed] == gold["norms"], (gold["norms"], printed[:6])


if __name__ == "__main__":
    worker()
