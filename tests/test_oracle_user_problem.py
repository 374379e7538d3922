"""The user-problem API (hpgmg_amd/problem.py, hpgmg_user_* of include/hpgmg_fv.h) on the CPU oracle.

The operator on dense arrays is checked against an independent SciPy assembly of operators.7pt.c + boundary_fd.c p1 (user_problem_lib.py),
solves against a direct solve, and the benchmark's own problem -- handed over as dense arrays -- against the benchmark's solve, bit for bit.
"""
import ctypes
import importlib.util
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend, VARIANTS, load_golden, split_variant
from user_problem_lib import assemble, benchmark_arrays, random_coefficients

SMOOTHER_NAME = {H.SMOOTH_CHEBY: "cheby", H.SMOOTH_GSRB: "gsrb", H.SMOOTH_JACOBI: "jacobi"}
GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8


@pytest.fixture(scope="module")
def lib():
    return Backend.oracle().lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_apply_matches_scipy_assembly(lib, n, box_dim, bc, a):
    alpha, bi, bj, bk = random_coefficients(n, bc, a != 0.0, seed=n + 7 * (bc == "periodic") + int(10 * a))
    b, h = 0.7, 1.0 / n
    x = np.random.default_rng(11).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, bc=bc, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        y = s.apply(x)
    ref = (assemble(n, bc, a, b, h, alpha, bi, bj, bk) @ x.ravel()).reshape(n, n, n)
    assert _rel(y, ref) <= 1e-13


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_mg_solve_matches_direct_solve(lib, n, box_dim, bc, a):
    alpha, bi, bj, bk = random_coefficients(n, bc, a != 0.0, seed=3 * n + (bc == "periodic") + int(10 * a))
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(5).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, bc=bc, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="mg", rtol=1e-10)
    assert info.converged and info.residual < 1e-10 * info.norm_f
    A = assemble(n, bc, a, b, h, alpha, bi, bj, bk).tocsc()
    singular = bc == "periodic" and a == 0.0
    rhs = f - f.mean() if singular else f
    if singular:           # pin one cell to make the direct solve regular, then compare without the mean
        A = A.tolil(); A[0, :] = 0.0; A[0, 0] = 1.0; A = A.tocsc()
        rhs = rhs.ravel().copy(); rhs[0] = 0.0
    ref = spl.spsolve(A, rhs.ravel()).reshape(n, n, n)
    if singular:
        ref, u = ref - ref.mean(), u - u.mean()
        assert info.mean_shift != 0.0
    assert _rel(u, ref) <= 1e-8


BENCH_CASES = ["7pt-cheby", "7pt-cheby-helm", "7pt-gsrb", "7pt-jacobi", "7pt-cheby-periodic", "7pt-gsrb-periodic"]


@pytest.mark.parametrize("variant", BENCH_CASES)
def test_benchmark_problem_through_the_api(lib, variant):
    """initialize_problem's arrays through set_coefficients / solve(fmg): the benchmark's u, bit for bit, and the reference's norm line.
    (Periodic Helmholtz is left out on purpose: the benchmark shifts f's mean there too, the API only where A is singular.)"""
    base, bcc = split_variant(variant)
    cfg = VARIANTS[base]
    bc = "periodic" if bcc == H.BC_PERIODIC else "dirichlet"
    a = 1.0 if cfg["helmholtz"] else 0.0
    gold = load_golden("fcycle_norms.json")[f"{variant} 4 8"]["norms"][0]
    B = Backend(lib, "oracle")
    B.configure(**cfg)
    bench = B.solver(2, 16, bc=bcc)           # hpgmg-fv 4 8: 2^3 boxes of 16^3
    try:
        r_bench = bench.fmg(0)
        u_bench = bench.level(0).interior(H.VECTOR_U)
    finally:
        bench.destroy()
    arr = benchmark_arrays(lib, 2, 16, bc, a, 1.0)
    with Solver(32, box_dim=16, bc=bc, smoother=SMOOTHER_NAME[cfg["smoother"]], a=a, b=1.0, lib=lib) as s:
        s.set_coefficients(arr["alpha"], arr["beta_i"], arr["beta_j"], arr["beta_k"])
        u, info = s.solve(arr["f"], method="fmg", rtol=1e-10)
    assert np.array_equal(u, u_bench)
    assert "%1.15e" % info.residual == "%1.15e" % r_bench == gold


def test_second_set_of_coefficients_equals_a_fresh_solver(lib):
    n, bc = 16, "dirichlet"
    first = random_coefficients(n, bc, True, seed=1)
    second = random_coefficients(n, bc, True, seed=2)
    f = np.random.default_rng(3).random((n, n, n))
    with Solver(n, box_dim=8, bc=bc, a=1.0, lib=lib) as s:
        s.set_coefficients(*first)
        s.solve(f)
        s.set_coefficients(*second)
        u1, _ = s.solve(f)
        y1 = s.apply(f)
    with Solver(n, box_dim=8, bc=bc, a=1.0, lib=lib) as s:
        s.set_coefficients(*second)
        u2, _ = s.solve(f)
        y2 = s.apply(f)
    assert np.array_equal(u1, u2) and np.array_equal(y1, y2)


def test_warm_start_from_a_converged_solution_takes_one_vcycle(lib):
    n, bc = 16, "dirichlet"
    coef = random_coefficients(n, bc, False, seed=4)
    f = np.random.default_rng(6).random((n, n, n))
    with Solver(n, box_dim=8, bc=bc, lib=lib) as s:
        s.set_coefficients(*coef)
        u, info = s.solve(f, method="mg", rtol=1e-10)
        assert info.converged and info.vcycles > 1
        out = np.empty_like(f)
        u2, info2 = s.solve(f, method="mg", rtol=1e-10, u0=u, out=out)
        assert u2 is out
        assert info2.vcycles == 1 and info2.converged
        assert np.abs(u2 - u).max() <= 1e-9 * np.abs(u).max()
        # a cold-ish start converges too, and u0 = 0 gives the same V-cycle count as no u0
        _, info3 = s.solve(f, method="mg", rtol=1e-10, u0=np.zeros_like(f))
        assert info3.converged and info3.vcycles == info.vcycles


def test_periodic_mean_shift_is_reported(lib):
    n = 16
    coef = random_coefficients(n, "periodic", False, seed=8)
    f = np.random.default_rng(9).random((n, n, n)) + 0.25
    with Solver(n, box_dim=8, bc="periodic", lib=lib) as s:
        s.set_coefficients(*coef)
        _, info = s.solve(f, method="mg")
        assert info.mean_shift == pytest.approx(f.mean(), rel=1e-12)
        assert info.converged
    with Solver(n, box_dim=8, bc="periodic", a=1.0, lib=lib) as s:      # a alpha term: nothing to shift
        s.set_coefficients(np.ones((n, n, n)), *coef[1:])
        _, info = s.solve(f, method="mg")
        assert info.mean_shift == 0.0


def test_bad_input_is_a_status_not_an_abort(lib):
    n, bc = 16, "dirichlet"
    alpha, bi, bj, bk = random_coefficients(n, bc, False, seed=10)
    f = np.ones((n, n, n))
    with Solver(n, box_dim=8, bc=bc, lib=lib) as s:
        neg = bj.copy(); neg[-1, -1, -1] = -1.0
        with pytest.raises(ValueError, match="beta_j"):
            s.set_coefficients(None, bi, neg, bk)
        with pytest.raises(ValueError, match="no valid coefficients"):        # the operator was half replaced: refused until a good set
            s.solve(f)
        nan = bk.copy(); nan[3, 4, 5] = np.nan
        with pytest.raises(ValueError, match="beta_k.*not finite"):
            s.set_coefficients(None, bi, bj, nan)
        zero = bi.copy(); zero[0, 0, 0] = 0.0
        with pytest.raises(ValueError, match="beta_i.*out of range"):
            s.set_coefficients(None, zero, bj, bk)
        s.set_coefficients(None, bi, bj, bk)
        bad_f = f.copy(); bad_f[-1, -1, -1] = np.nan
        with pytest.raises(ValueError, match="^f:"):
            s.solve(bad_f)
        with pytest.raises(ValueError, match="beta_i: shape"):
            s.set_coefficients(None, bj, bj, bk)                             # (N,N+1,N) where (N,N,N+1) belongs
        with pytest.raises(ValueError, match="f: shape"):
            s.solve(np.ones((n, n, n + 1)))
        with pytest.raises(ValueError, match="f: dtype"):
            s.solve(np.ones((n, n, n), dtype=np.float32))
        with pytest.raises(ValueError, match="alpha"):
            s.set_coefficients(np.ones((n, n, n)), bi, bj, bk)               # Poisson has no alpha
        with pytest.raises(ValueError, match="configured for another"):
            Solver(n, box_dim=8, bc=bc, smoother="gsrb", lib=lib)           # a live solver holds {7pt, Chebyshev, Poisson}
        with pytest.raises(ValueError, match="configured for another"):
            Solver(n, box_dim=8, bc=bc, a=1.0, lib=lib)
        u, info = s.solve(f)                                                # still usable
        assert np.isfinite(u).all() and info.vcycles >= 1
    with pytest.raises(ValueError, match="operator"):
        Solver(n, box_dim=8, operator="27pt", lib=lib)
    with pytest.raises(ValueError, match="box_dim"):
        Solver(n, box_dim=6, lib=lib)
    with Solver(n, box_dim=8, bc=bc, smoother="gsrb", lib=lib) as s:       # no live solver any more: another configuration is fine
        s.set_coefficients(None, bi, bj, bk)


def test_default_box_dim(lib):
    for n, want in ((16, 16), (24, 8), (48, 16)):
        with Solver(n, lib=lib) as s:
            info = (ctypes.c_int * H.INFO_COUNT)()
            lib.hpgmg_level_info(lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0), info)
            assert info[H.INFO_BOX_DIM] == want and info[H.INFO_DIM] == n


_CHILD = r"""
import os
import sys
sys.path.insert(0, {root!r})
order = sys.argv[1]
if order == "torch-first":
    import torch  # noqa: F401
import hpgmg_amd as H
H.load_driver()
if order == "libs-first":
    import torch  # noqa: F401
from hpgmg_amd.problem import check_single_hip_runtime, hip_runtimes_mapped
print(len(hip_runtimes_mapped()))
try:
    check_single_hip_runtime()
    print("guard: passed")
except RuntimeError as e:
    print("guard:", e)
sys.stdout.flush()
os._exit(0)            # two HIP runtimes in one process (libs-first) must not both run their exit-time teardown
"""


@pytest.mark.parametrize("order", ["torch-first", "libs-first"])
def test_one_hip_runtime_when_torch_comes_first(order):
    if importlib.util.find_spec("torch") is None:      # looked up, not imported: torch in THIS process would be a second HIP runtime
        pytest.skip("torch is not installed")
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), order], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    if order == "torch-first":
        assert lines[0] == "1" and lines[1] == "guard: passed", out.stdout
    else:
        assert int(lines[0]) > 1 and "import torch before hpgmg_amd" in lines[1], out.stdout
