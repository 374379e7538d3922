"""The sweep-pair kernel may form Dinv in registers instead of reading VECTOR_DINV (kernels/cheby_pair.hpp: PairArgs.form_dinv,
HPGMG_PAIR_FORM_DINV / hpgmg_set_pair_form_dinv).  The stored vector is the contract: whichever form runs, the bits are those of the
oracle, which always reads the vector.  Every comparison here is bit for bit; hpgmg_pair_formed_dinv_launches() says which form ran.

The waves per workgroup are chosen once per process (HPGMG_TUNE_PAIR_NW), so the smooth() cases run in a worker process per wave count: this
file run as a script does all of them and prints one JSON line each.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (the OpenMP environment of the suite, before any runtime loads)

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, Backend, load_golden
from test_gpu_operators import make_pair

pytestmark = pytest.mark.gpu

# name -> variant, (boxes per side, box side): one box of 128^3 (every wall flag; lanes 0 and 63 both on walls), 128^3 in boxes of 64 (the NARROW
# instance: box faces inside a row are no walls), 2^3 boxes of 128^3 (an interior tile edge in i: lane 0 / 63 not on a wall; two k chunks)
CASES = {
    "helm-1x128": ("7pt-cheby-helm", (1, 128)), "cheby-1x128": ("7pt-cheby", (1, 128)), "gsrb-1x128": ("7pt-gsrb", (1, 128)),
    "helm-2x64": ("7pt-cheby-helm", (2, 64)), "cheby-2x64": ("7pt-cheby", (2, 64)), "gsrb-2x64": ("7pt-gsrb", (2, 64)),
    "helm-2x128": ("7pt-cheby-helm", (2, 128)),
}
OUT = (H.VECTOR_U, H.VECTOR_TEMP)


def declare(lib):
    lib.hpgmg_set_pair_form_dinv.argtypes = [ctypes.c_int]
    lib.hpgmg_pair_formed_dinv_launches.restype = ctypes.c_longlong
    lib.hpgmg_set_pair_min_cells.argtypes = [ctypes.c_longlong]
    return lib


def coefficients_of(variant):
    return (1.0, 1.0) if "helm" in variant else (0.0, 1.0)


def smooth_and_read(lv, a, b):
    lv.b.lib.smooth(lv.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
    return [lv.interior(v) for v in OUT]


def equal(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def smooth_case(hip, oracle, variant, geom):
    """smooth() after rebuild_operator on seeded coefficients: formed, loaded and the oracle's four sweeps."""
    lib = hip.lib
    lh, lo = make_pair(hip, oracle, variant, *geom, seed=7)
    try:
        a, b = coefficients_of(variant)
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, a, b)
        start = [lh.read_all(v) for v in OUT]
        lib.hpgmg_set_pair_form_dinv(1)
        n0 = lib.hpgmg_pair_formed_dinv_launches()
        formed = smooth_and_read(lh, a, b)
        n1 = lib.hpgmg_pair_formed_dinv_launches()
        for v, data in zip(OUT, start):
            lh.write_all(v, data)
        lib.hpgmg_set_pair_form_dinv(0)
        loaded = smooth_and_read(lh, a, b)
        n2 = lib.hpgmg_pair_formed_dinv_launches()
        ref = smooth_and_read(lo, a, b)
        sha = hashlib.sha256(b"".join(x.tobytes() for x in formed)).hexdigest()
        return {"formed_is_loaded": equal(formed, loaded), "formed_is_oracle": equal(formed, ref), "rise_on": n1 - n0, "rise_off": n2 - n1, "sha": sha}
    finally:
        lib.hpgmg_set_pair_form_dinv(1)
        lh.destroy(); lo.destroy()


def worker():
    hip, oracle = Backend.hip(), Backend.oracle()
    declare(hip.lib)
    hip.lib.hpgmg_set_pair_min_cells(1 << 20)
    for name, (variant, geom) in CASES.items():
        print("CASE " + json.dumps(dict(smooth_case(hip, oracle, variant, geom), case=name)), flush=True)


_RUNS = {}


def run_with(nw):
    if nw not in _RUNS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=900,
                             env=dict(os.environ, HPGMG_TUNE_PAIR_NW=str(nw)))
        assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
        rows = [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CASE ")]
        _RUNS[nw] = {r["case"]: r for r in rows}
        assert sorted(_RUNS[nw]) == sorted(CASES)
    return _RUNS[nw]


@pytest.mark.parametrize("nw", [10, 12, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_smooth_forms_the_stored_bits(case, nw):
    """10 and 12 waves form Dinv (two launches per smooth()), 16 waves read it; the switch off: nobody forms.  All equal the oracle, and each other."""
    r = run_with(nw)[case]
    print(case, nw, r)
    assert r["formed_is_loaded"] and r["formed_is_oracle"]
    assert r["rise_off"] == 0
    assert r["rise_on"] == (0 if nw == 16 else 2)
    assert r["sha"] == run_with(10)[case]["sha"]


def test_the_guards(hip, oracle):
    """Whenever VECTOR_DINV may not be what rebuild_operator made of the coefficient vectors for the a, b of the call, the launch reads it."""
    lib = declare(hip.lib)
    lib.hpgmg_set_pair_form_dinv(1)
    lh, lo = make_pair(hip, oracle, "7pt-cheby-helm", 1, 128, seed=11)
    formed = lib.hpgmg_pair_formed_dinv_launches

    def check(a, b, rise):
        n0 = formed()
        got, ref = smooth_and_read(lh, a, b), smooth_and_read(lo, a, b)
        assert equal(got, ref)
        assert formed() - n0 == rise

    try:
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, 1.0, 1.0)
        check(1.0, 1.0, 2)
        check(2.0, 1.0, 0)                                   # another a than the rebuild's
        check(1.0, 0.5, 0)                                   # another b
        check(1.0, 1.0, 2)
        stale = np.abs(lh.read_all(H.VECTOR_DINV)) * 0.75    # VECTOR_DINV overwritten after the rebuild
        for lv in (lh, lo):
            lv.write_all(H.VECTOR_DINV, stale)
        check(1.0, 1.0, 0)
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, 1.0, 1.0)
        check(1.0, 1.0, 2)
        beta = np.abs(lh.read_all(H.VECTOR_BETA_J)) + 0.25   # a coefficient vector overwritten without a new rebuild
        for lv in (lh, lo):
            lv.write_all(H.VECTOR_BETA_J, beta)
        check(1.0, 1.0, 0)
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, 1.0, 1.0)
        check(1.0, 1.0, 2)
    finally:
        lh.destroy(); lo.destroy()


@pytest.mark.parametrize("size", ["6 8", "7 1"])
def test_the_fold_prints_the_same_lines(size):
    """hpgmg-fv --helmholtz with fine levels of 128^3: the up-leg's smooth() takes the INTERP instances.  Switch on and off print the same pinned lines,
    and the f-cycle norms are the golden ones where the reference's are recorded."""
    import re
    from test_gpu_parity_sweep import pinned_lines
    exe = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")
    on = pinned_lines(exe, "--helmholtz", size, HPGMG_PAIR_FORM_DINV="1")
    off = pinned_lines(exe, "--helmholtz", size, HPGMG_PAIR_FORM_DINV="0")
    assert len(on) >= 10 and on == off
    gold = load_golden("fcycle_norms.json").get("7pt-cheby-helm " + size)
    if gold:
        printed = [re.search(r"norm=(\S+)", l).group(1) for l in on if "f-cycle" in l]
        assert [g for g in gold["norms"] if g in printed] == gold["norms"], (gold["norms"], printed[:6])


def test_dense_array_solver_with_neumann_and_robin_walls():
    """n = 128, one Neumann and one Robin wall, Dirichlet elsewhere: the wall betas change BEFORE rebuild_operator, so the formed Dinv is the stored one."""
    from hpgmg_amd.problem import Solver
    from user_problem_lib import random_coefficients
    from user_robin_lib import D, N, R, kappa_of
    n, faces = 128, (D, N, D, R, D, D)
    hip, oracle = declare(Backend.hip().lib), Backend.oracle().lib
    assert H.load_kernels().hpgmg_hip_set_device(0) == 0
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", True, seed=1280)
    rng = np.random.default_rng(n)
    f, g, kappa = rng.random((n, n, n)) - 0.3, rng.random((6, n, n)) * 4.0 - 2.0, kappa_of(n, faces)

    def fcycle(lib):
        lib.hpgmg_set_verbose(0)
        u, info, shift = np.empty((n, n, n)), H.UserInfo(), ctypes.c_double()
        with Solver(n, box_dim=64, bc=faces, smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
            S = s._ptr
            assert lib.hpgmg_user_set_coefficients_robin(S, alpha.ctypes.data, bi.ctypes.data, bj.ctypes.data, bk.ctypes.data, kappa.ctypes.data, H.WHERE_HOST) == 0
            assert lib.hpgmg_user_set_rhs_dirichlet(S, f.ctypes.data, g.ctypes.data, H.WHERE_HOST, ctypes.byref(shift)) == 0
            assert lib.hpgmg_user_solve(S, H.USER_FMG, 1.0, None, H.WHERE_HOST, ctypes.byref(info)) == 0      # rtol 1: the F-cycle alone
            assert lib.hpgmg_user_get_solution(S, u.ctypes.data, H.WHERE_HOST) == 0
        return u, info.norm_of_residual

    try:
        hip.hpgmg_set_pair_form_dinv(1)
        n0 = hip.hpgmg_pair_formed_dinv_launches()
        on = fcycle(hip)
        assert hip.hpgmg_pair_formed_dinv_launches() > n0
        hip.hpgmg_set_pair_form_dinv(0)
        n1 = hip.hpgmg_pair_formed_dinv_launches()
        off = fcycle(hip)
        assert hip.hpgmg_pair_formed_dinv_launches() == n1
    finally:
        hip.hpgmg_set_pair_form_dinv(1)
    ref = fcycle(oracle)
    assert on[0].tobytes() == off[0].tobytes() == ref[0].tobytes()
    assert on[1] == off[1] == ref[1]


if __name__ == "__main__":
    worker()
