"""Solver.eigs (hpgmg_user_eigs) on the MI355X against the CPU oracle, bit for bit: lam, the modes, EigInfo.residuals, mu, the
iteration and V-cycle counts.  The host driver is the same C on both sides, the three block hooks are bit-identical (tests/test_gpu_block_hooks.py) and
the V-cycle is held to the oracle elsewhere, so a difference is a bug, not noise.

| case | what it reaches |
|---|---|
| N = 16, boxes of 8, Dirichlet Poisson | 8 boxes of one partial column block; M = I, no weight stream |
| N = 24, boxes of 8, mixed Robin / Neumann / Dirichlet walls, a = 1.3 | 27 boxes, an odd factor: BiCGStab at the bottom |
| N = 32, boxes of 16, periodic Helmholtz | the wrap; one full segment |
| N = 64, boxes of 32, contrast 100, k = 3 | two segments, four column blocks; the sweep-pair and brick paths of the V-cycle |
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import user_eigs_lib as E
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT

pytestmark = pytest.mark.gpu
CASES = [("poisson", 16, 8, 4), ("corners", 24, 8, 3), ("periodic", 32, 16, 4), ("contrast", 64, 32, 3)]


@pytest.fixture(scope="module")
def libs(hip, oracle):
    return hip.lib, oracle.lib


@pytest.mark.parametrize("name,n,box,k", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_eigs_equals_the_oracle(libs, name, n, box, k):
    out = []
    for lib in libs:
        with Solver(n, box_dim=box, bc=E.bc_of(name), a=E.CASES[name][1], b=E.B, lib=lib) as s:
            E.set_case(s, name, n)
            out.append(s.eigs(k, rtol=1e-6))
    (lam_h, modes_h, info_h), (lam_o, modes_o, info_o) = out
    print(f"{name} N={n}: iterations hip {info_h.iterations} oracle {info_o.iterations}; vcycles {info_h.vcycles} {info_o.vcycles}; lam hip {lam_h} oracle {lam_o}; "
          f"residuals hip {info_h.residuals} oracle {info_o.residuals}; modes differ in {int((modes_h.view(np.uint64) != modes_o.view(np.uint64)).sum())} doubles")
    assert info_o.converged and info_h.converged
    assert (info_h.iterations, info_h.vcycles) == (info_o.iterations, info_o.vcycles)
    assert lam_h.tobytes() == lam_o.tobytes() and info_h.mu.tobytes() == info_o.mu.tobytes() and info_h.residuals.tobytes() == info_o.residuals.tobytes()
    assert modes_h.tobytes() == modes_o.tobytes()


def test_start_block_out_and_lifecycle(libs):
    """x0= and out= on the host path, the same call twice, and a solve after eigs: HIP as the oracle, byte for byte."""
    n, k = 16, 2
    rng = np.random.default_rng(11)
    x0, f = rng.random((k + 2, n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5
    out = []
    for lib in libs:
        with Solver(n, box_dim=8, bc=E.bc_of("neumann"), a=0.9, b=E.B, lib=lib) as s:
            E.set_case(s, "neumann", n)
            into = np.full((k, n, n, n), np.nan)
            lam, modes, info = s.eigs(k, rtol=1e-6, x0=x0, out=into)
            assert modes is into and info.converged
            again = s.eigs(k, rtol=1e-6, x0=x0)
            assert again[1].tobytes() == into.tobytes() and again[0].tobytes() == lam.tobytes()
            u, _ = s.solve(f, method="mg", rtol=1e-9)
            out.append((lam, modes, info, u))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes() and out[0][3].tobytes() == out[1][3].tobytes()
    assert out[0][2].iterations == out[1][2].iterations and out[0][2].residuals.tobytes() == out[1][2].residuals.tobytes()


def test_torch_tensors(libs):
    """A child process that imports torch first: eigs on device tensors (x0=, out=) gives the bytes of the host path and writes out= in place."""
    worker = os.path.join(ROOT, "tests", "user_eigs_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
