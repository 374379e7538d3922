"""Robin (convective) walls of the user-problem API (Solver(n, bc=<6-tuple with "convective">), set_coefficients(..., robin=kappa),
hpgmg_user_set_coefficients_robin) on the CPU oracle.  DESIGN.md §11.5.

apply(x, boundary=g) is checked against a SciPy assembly of A_R x - T(g) and V-cycle solves against a direct solve; kappa = 0 against the
Neumann solver bit for bit; six Robin walls against the singular path; every level's wall coefficients against the formula with that level's
h; kappa -> infinity against the Dirichlet solver; the interpolation correction alone on a linear u; and on a manufactured solution the order
of the V-cycle error, the FMG property of the F-cycle and the V-cycle counts next to Dirichlet walls.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_boundary_lib import exact, manufactured
from user_neumann_lib import grad_exact
from user_pcg_lib import contrast_problem
from user_problem_lib import random_coefficients
from user_robin_lib import (ALL, CORNERS, SIDES, WALLS, assemble_robin, beta_cells, kappa_field, kappa_of, level_vector, level_walls, levels_of,
                            lift_robin, mask_of, neumann_of, restrict_faces, sample_faces, wall_array, wall_entries)

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8
# the project's gates (test_oracle_user_boundary.py, test_oracle_user_neumann.py).  Measured with Robin walls: the table of DESIGN.md §11.5
FMG_FACTOR = 1.5
ORDER_FACTOR = 3.0
VCYCLE_MARGIN = 4
MGPCG_ITERATIONS = {"cheby": 28}        # test_oracle_user_pcg.py's gate on the contrast problem (N = 32, contrast 100, rtol 1e-8), before its 25 %


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


def _random_boundary(n, seed):
    return np.random.default_rng(seed).random((6, n, n)) * 4.0 - 2.0


def _packed_f(lib, s):
    F = np.empty((s.n,) * 3)
    assert lib.hpgmg_dense_unpack(levels_of(lib, s)[0], H.VECTOR_F, F.ctypes.data, H.WHERE_HOST) == 0
    return F


# ---------------------------------------------------------------- assembly
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
@pytest.mark.parametrize("walls", ["one", "sides", "all", "corners"])
def test_apply_matches_scipy_assembly(lib, walls, n, box_dim, a):
    faces = WALLS[walls]
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=100 + n + int(10 * a))
    b, h = 0.7, 1.0 / n
    kappa = kappa_of(n, faces)
    x = np.random.default_rng(12).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 13)
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk, robin=kappa)
        y = s.apply(x, boundary=g)
        y0 = s.apply(x)
        yz = s.apply(x, boundary=np.zeros((6, n, n)))
    A = assemble_robin(n, faces, kappa, a, b, h, alpha, bi, bj, bk)
    ref = (A @ x.ravel()).reshape(n, n, n) - lift_robin(n, faces, kappa, b, h, bi, bj, bk, g)
    assert _rel(y, ref) <= 1e-13
    assert not np.array_equal(y, y0)
    assert np.array_equal(yz, y0)                              # boundary=None is zero data


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
@pytest.mark.parametrize("walls", ["one", "sides", "all", "corners"])
def test_mg_solve_matches_direct_solve(lib, walls, n, box_dim, a):
    faces = WALLS[walls]
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=200 + n + int(10 * a))
    b, h = 1.0, 1.0 / n
    kappa = kappa_of(n, faces)
    f = np.random.default_rng(7).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 8)
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk, robin=kappa)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        r = s.apply(u, boundary=g) - f
    assert info.converged and info.mean_shift == 0.0
    F = f + lift_robin(n, faces, kappa, b, h, bi, bj, bk, g)
    assert info.norm_f == pytest.approx(np.abs(F).max(), rel=1e-14)
    ref = spl.spsolve(assemble_robin(n, faces, kappa, a, b, h, alpha, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8
    assert np.abs(r).max() <= 1e-10 * np.abs(F).max()


# ---------------------------------------------------------------- kappa = 0 is the Neumann wall
def _everything(lib, s, f, g, x):
    out = []
    for method in ("fmg", "mg"):
        u, info = s.solve(f, method=method, boundary=g)
        out += [u, np.array([info.residual, info.norm_f, info.vcycles, info.mean_shift])]
        if method == "fmg":
            out.append(_packed_f(lib, s))
    out.append(s.apply(x, boundary=g))
    u, info = s.solve(f)                                       # zero data
    out += [u, np.array([info.residual, info.norm_f, info.vcycles, info.mean_shift])]
    for vecs, eig in level_walls(lib, s):
        out.append(np.array([eig]))
        out += [v for per_vector in vecs for _, v in per_vector]
    out.append(np.array([lib.hpgmg_level_must_subtract_mean(L) for L in levels_of(lib, s)], dtype=np.float64))
    return out


@pytest.mark.parametrize("walls,a,smoother", [("corners", 1.0, "cheby"), ("sides", 0.0, "gsrb"), ("all", 0.0, "cheby"), ("all", 1.0, "jacobi")])
def test_kappa_zero_is_the_neumann_solver_bit_for_bit(lib, walls, a, smoother):
    n, faces = 16, WALLS[walls]
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=310 + len(smoother))
    rng = np.random.default_rng(31)
    f, x, g = rng.random((n, n, n)) - 0.4, rng.random((n, n, n)) * 2.0 - 1.0, _random_boundary(n, 32)
    with Solver(n, box_dim=8, bc=neumann_of(faces), smoother=smoother, a=a, lib=lib) as s:
        s.set_coefficients(*coef)
        ref = _everything(lib, s, f, g, x)
    for robin in (np.zeros((6, n, n)), [0.0] * 6):
        with Solver(n, box_dim=8, bc=faces, smoother=smoother, a=a, lib=lib) as s:
            s.set_coefficients(*coef, robin=robin)
            got = _everything(lib, s, f, g, x)
        assert len(got) == len(ref)
        for i, (p, q) in enumerate(zip(got, ref)):
            assert p.tobytes() == q.tobytes(), i
    if walls == "all" and a == 0.0:
        assert ref[1][3] != 0.0 and np.all(ref[-1] == 1.0)     # the singular path: a mean shift, every level mean-free


@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_six_robin_walls_are_not_singular(lib, n, box_dim):
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=250 + n)
    b, h = 1.0, 1.0 / n
    kappa = kappa_of(n, ALL)
    f = np.random.default_rng(17).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 18)
    with Solver(n, box_dim=box_dim, bc=ALL, a=0.0, b=b, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk, robin=kappa)
        shift = s.set_rhs(f, boundary=g)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        u_f, info_f = s.solve(f, method="fmg", boundary=g)
        assert [lib.hpgmg_level_must_subtract_mean(L) for L in levels_of(lib, s)] == [0] * len(levels_of(lib, s))
        s.set_coefficients(None, bi, bj, bk, robin=[0.0] * 6)                  # and back: kappa = 0 everywhere is singular again
        assert [lib.hpgmg_level_must_subtract_mean(L) for L in levels_of(lib, s)] == [1] * len(levels_of(lib, s))
        assert s.set_rhs(f, boundary=g) != 0.0
    assert shift == 0.0 and info.mean_shift == 0.0 and info_f.mean_shift == 0.0
    assert info.converged and info_f.vcycles == 1
    F = f + lift_robin(n, ALL, kappa, b, h, bi, bj, bk, g)
    ref = spl.spsolve(assemble_robin(n, ALL, kappa, 0.0, b, h, None, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8


# ---------------------------------------------------------------- coarse operators
@pytest.mark.parametrize("walls", ["one", "sides", "all", "corners"])
@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_every_level_has_its_own_wall_coefficient(lib, walls, n, box_dim):
    """On the masked walls wall_l * (t / (2.0 + t)), t = kappa_l * h_l, bit for bit (0.0 on a Neumann wall); elsewhere the all-Dirichlet solver's beta."""
    faces = WALLS[walls]
    coef = random_coefficients(n, "dirichlet", True, seed=350 + n)
    kappa = kappa_of(n, faces)
    with Solver(n, box_dim=box_dim, bc=faces, a=1.0, lib=lib) as s, Solver(n, box_dim=box_dim, a=1.0, lib=lib) as d:
        s.set_coefficients(*coef, robin=kappa)
        d.set_coefficients(*coef)
        Ls, Ld = levels_of(lib, s), levels_of(lib, d)
        levels = min(len(Ls), len(Ld))
        assert levels >= 3
        wall_l, kappa_l, walls_seen = wall_array(n, *coef[1:]), kappa, 0
        for l in range(levels):
            if l:
                wall_l, kappa_l = restrict_faces(wall_l), restrict_faces(kappa_l)
            h_l = lib.hpgmg_level_h(Ls[l])
            assert h_l == (1.0 / n) * 2 ** l
            t = kappa_l * h_l
            expect_wall = wall_l * (t / (2.0 + t))
            for axis, vid in enumerate((H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)):
                info, got = level_vector(lib, Ls[l], vid)
                _, ref = level_vector(lib, Ld[l], vid)
                nl, dim = info[H.INFO_DIM], info[H.INFO_BOX_DIM]
                idx = beta_cells(info, axis)
                for (low, v), (low_d, vd) in zip(got, ref):
                    assert low == low_d
                    expect = vd[idx].copy()
                    assert (expect > 0.0).all()
                    for side, at, on_wall in ((0, 0, low[axis] == 0), (1, dim, low[axis] + dim == nl)):
                        face = 2 * axis + side
                        if faces[face] != "dirichlet" and on_wall:
                            expect[at] = wall_entries(expect_wall, face, low, dim)
                            assert (expect[at] > 0.0).all() if faces[face] == "convective" else (expect[at] == 0.0).all()
                            walls_seen += 1
                    assert v[idx].tobytes() == expect.tobytes(), (l, axis, low)
        assert walls_seen >= levels * bin(mask_of(faces)).count("1")


# ---------------------------------------------------------------- the Dirichlet limit
def test_large_kappa_is_the_dirichlet_wall(lib):
    """kappa = 1e10 with g = kappa g_D: the wall coefficient differs from Dirichlet's by 4 / (2 + kappa h) = 6e-9 relative."""
    n, big = 16, 1e10
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=420)
    f = np.random.default_rng(42).random((n, n, n)) * 2.0 - 1.0
    g_d = _random_boundary(n, 43)
    with Solver(n, box_dim=8, bc="dirichlet", lib=lib) as d:
        d.set_coefficients(None, bi, bj, bk)
        u_d, info_d = d.solve(f, method="mg", rtol=1e-12, boundary=g_d)
    with Solver(n, box_dim=8, bc=ALL, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk, robin=[big] * 6)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=big * g_d)
    assert info.converged and info_d.converged
    print(f"kappa = 1e10 against Dirichlet: {_rel(u, u_d):.3e}")
    assert _rel(u, u_d) <= 1e-6


# ---------------------------------------------------------------- the F-cycle's interpolation correction
def _linear(x, y, z):
    return 0.3 + 1.1 * x - 0.7 * y + 0.5 * z


def _linear_grad(x, y, z):
    return 1.1 + 0.0 * x, -0.7 + 0.0 * x, 0.5 + 0.0 * x


@pytest.mark.parametrize("walls", ["one", "sides", "all", "corners"])
def test_interpolation_correction_reproduces_a_linear_function(lib, walls):
    """interpolation_fcycle (p1) from level l+1 plus the hook's correction gives a linear u on level l to rounding, on faces, edges and corners."""
    n, faces = 16, WALLS[walls]
    with Solver(n, box_dim=8, bc=faces, lib=lib) as s:
        levels = levels_of(lib, s)
        for l in (0, 1):
            Lf, Lc = levels[l], levels[l + 1]
            nf, nc = n >> l, n >> (l + 1)
            cf, cc = (np.arange(nf) + 0.5) / nf, (np.arange(nc) + 0.5) / nc
            Z, Y, X = np.meshgrid(cc, cc, cc, indexing="ij")
            uc = np.ascontiguousarray(_linear(X, Y, Z))
            kc = kappa_of(nc, faces)                            # any kappa >= 0 of the coarse level, with the data that belongs to it
            with Solver(nc, box_dim=4, bc=faces, h=1.0 / nc, lib=lib) as sampler:
                gc = sampler.boundary_from(_linear, grad=_linear_grad, robin=kc)
            zero = np.zeros((nf, nf, nf))
            assert lib.hpgmg_dense_pack(Lc, H.VECTOR_U, uc.ctypes.data, H.WHERE_HOST, 0, 0) == 0
            assert lib.hpgmg_dense_pack(Lf, H.VECTOR_U, zero.ctypes.data, H.WHERE_HOST, 0, 0) == 0
            lib.interpolation_fcycle(Lf, H.VECTOR_U, 0.0, Lc, H.VECTOR_U)
            plain = np.empty((nf, nf, nf))
            assert lib.hpgmg_dense_unpack(Lf, H.VECTOR_U, plain.ctypes.data, H.WHERE_HOST) == 0
            lib.hpgmg_boundary_interp_robin(Lf, H.VECTOR_U, Lc, gc.ctypes.data, mask_of(faces), kc.ctypes.data)
            got = np.empty((nf, nf, nf))
            assert lib.hpgmg_dense_unpack(Lf, H.VECTOR_U, got.ctypes.data, H.WHERE_HOST) == 0
            Z, Y, X = np.meshgrid(cf, cf, cf, indexing="ij")
            ref = _linear(X, Y, Z)
            print(f"{walls} level {l}: linear u after the correction, max error {np.abs(got - ref).max():.3e}")
            assert np.abs(got - ref).max() <= 1e-14, (l, np.abs(got - ref).max())
            shell = np.ones_like(ref, dtype=bool)
            shell[1:-1, 1:-1, 1:-1] = False
            assert np.array_equal(got[~shell], plain[~shell])                # only boundary cells are touched
            assert np.abs(plain - ref)[shell].max() > 0.1                      # which the homogeneous ghosts leave far off


# ---------------------------------------------------------------- order, FMG property, V-cycle counts
_ERRORS = {}


def _errors(lib, n, a, walls):
    """(V-cycle error, F-cycle error) against u* of user_boundary_lib.manufactured, computed once per case."""
    key = (n, a, walls)
    if key not in _ERRORS:
        faces = WALLS[walls]
        alpha, bi, bj, bk, f, u_star = manufactured(n, a, 1.0)
        kappa = kappa_of(n, faces)
        with Solver(n, box_dim=min(n // 2, 32), bc=faces, a=a, b=1.0, lib=lib) as s:
            s.set_coefficients(alpha, bi, bj, bk, robin=kappa)
            g = s.boundary_from(exact, grad=grad_exact, robin=kappa)
            assert np.all(np.abs(g) > 1e-3)                    # non-zero data on every face
            u_mg, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
            u_fmg, info_f = s.solve(f, method="fmg", boundary=g)
            assert info.converged and info_f.vcycles == 1 and info.mean_shift == 0.0
        _ERRORS[key] = (np.abs(u_mg - u_star).max(), np.abs(u_fmg - u_star).max())
    return _ERRORS[key]


CYCLE_CASES = [("one", 1.0), ("sides", 1.0), ("sides", 0.0), ("all", 1.0), ("all", 0.0), ("corners", 0.0)]


@pytest.mark.parametrize("walls,a", CYCLE_CASES)
def test_manufactured_solution_is_second_order(lib, walls, a):
    errs = [_errors(lib, n, a, walls)[0] for n in (16, 32, 64)]
    factors = [errs[i] / errs[i + 1] for i in range(2)]
    print(f"{walls} a={a}: V-cycle errors {errs}, factors {factors}")
    assert min(factors) >= ORDER_FACTOR, (errs, factors)


@pytest.mark.parametrize("walls,a", CYCLE_CASES)
def test_one_fcycle_is_as_accurate_as_vcycles(lib, walls, a):
    for n in (16, 32, 64):
        e_mg, e_fmg = _errors(lib, n, a, walls)
        print(f"{walls} a={a} N={n}: V-cycles {e_mg:.3e}; F-cycle {e_fmg:.3e}, {e_fmg / e_mg:.3f}x")
        assert e_fmg <= FMG_FACTOR * e_mg, (n, e_fmg, e_mg)


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("smoother", ["cheby", "gsrb", "jacobi"])
@pytest.mark.parametrize("a", [0.0, 1.0])
def test_vcycle_count_next_to_dirichlet_walls(lib, smoother, a, n):
    alpha, bi, bj, bk, f, _ = manufactured(n, a, 1.0)
    counts = {}
    for name, faces in (("dirichlet", "dirichlet"),) + tuple(WALLS.items()):
        robin = kappa_of(n, faces) if name != "dirichlet" else None
        with Solver(n, box_dim=16, bc=faces, smoother=smoother, a=a, b=1.0, lib=lib) as s:
            s.set_coefficients(alpha, bi, bj, bk, robin=robin)
            g = s.boundary_from(exact, grad=grad_exact, robin=robin)
            _, info = s.solve(f, method="mg", rtol=1e-10, boundary=g)
            assert info.converged
            counts[name] = info.vcycles
    print(f"N={n} {smoother} a={a}: V-cycles to 1e-10 {counts}")
    for name in WALLS:
        assert counts[name] <= counts["dirichlet"] + VCYCLE_MARGIN, counts


@pytest.mark.parametrize("method", ["pcg", "fpcg"])
def test_cg_on_the_contrast_problem_with_robin_walls(lib, method):
    n = 32
    bi, bj, bk, f = contrast_problem(n, 100.0)
    kappa = kappa_of(n, SIDES)
    with Solver(n, box_dim=16, bc=SIDES, smoother="cheby", lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk, robin=kappa)
        u, info = s.solve(f, method=method, rtol=1e-8, max_iter=50)
        r = np.abs(s.apply(u, boundary=np.zeros((6, n, n))) - f).max()
    print(f"contrast 100, Robin side walls, {method}: {info.vcycles} iterations, rel {info.residual / info.norm_f:.3e}")
    assert info.converged and info.residual < 1e-8 * info.norm_f
    assert info.vcycles <= 1.25 * MGPCG_ITERATIONS["cheby"]
    assert abs(r - info.residual) <= 1e-12 * r


# ---------------------------------------------------------------- the Python layer
def test_boundary_from_samples_the_robin_data(lib):
    n, h = 8, 0.5
    kappa = [2.0, 0.0, 0.0, 3.0, 0.0, 0.0]
    with Solver(n, box_dim=4, bc=CORNERS, h=h, lib=lib) as s:
        g = s.boundary_from(lambda x, y, z: x + 10.0 * y + 100.0 * z, grad=lambda x, y, z: (1.0 + 0 * x, 10.0 + 0 * x, 100.0 + 0 * x), robin=kappa)
        full = s.boundary_from(lambda x, y, z: x + 10.0 * y + 100.0 * z, grad=lambda x, y, z: (1.0 + 0 * x, 10.0 + 0 * x, 100.0 + 0 * x),
                               robin=np.broadcast_to(np.array(kappa)[:, None, None], (6, n, n)).copy())
    c = (np.arange(n) + 0.5) * h
    assert np.array_equal(g, full)
    assert np.array_equal(g[0], -1.0 + 2.0 * (10.0 * c[None, :] + 100.0 * c[:, None]))      # i-low, Robin: -du/dx + kappa u
    assert np.array_equal(g[1], n * h + 10.0 * c[None, :] + 100.0 * c[:, None])             # i-high, Dirichlet: u
    assert np.array_equal(g[2], np.full((n, n), -10.0))                                     # j-low, Neumann: -du/dy
    assert np.array_equal(g[3], 10.0 + 3.0 * (c[None, :] + 10.0 * n * h + 100.0 * c[:, None]))   # j-high, Robin: +du/dy + kappa u
    assert np.array_equal(g[4], np.full((n, n), -100.0))                                    # k-low, Robin with kappa = 0: -du/dz


def test_six_numbers_are_broadcast_per_face(lib):
    n = 16
    coef = random_coefficients(n, "dirichlet", False, seed=500)
    x = np.random.default_rng(50).random((n, n, n))
    values = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    with Solver(n, box_dim=8, bc=CORNERS, lib=lib) as s:
        s.set_coefficients(*coef, robin=values)
        y = s.apply(x)
        junk = np.broadcast_to(np.array(values)[:, None, None], (6, n, n)).copy()
        for f, kind in enumerate(CORNERS):
            if kind != "convective":
                junk[f] = -5.0                                 # entries of faces that are not Robin are not read
        s.set_coefficients(*coef, robin=junk)
        assert np.array_equal(s.apply(x), y)


def test_refusals(lib):
    n = 16
    coef = random_coefficients(n, "dirichlet", False, seed=400)
    f = np.ones((n, n, n))
    kappa = kappa_of(n, SIDES)
    with pytest.raises(ValueError, match="^bc:.*periodic"):
        Solver(n, box_dim=8, bc=("periodic", "periodic") + ("convective",) * 4, lib=lib)
    with pytest.raises(ValueError, match="^bc:"):
        Solver(n, box_dim=8, bc="convective", lib=lib)
    with Solver(n, box_dim=8, bc=SIDES, lib=lib) as s:
        with pytest.raises(ValueError, match="^robin:.*required"):
            s.set_coefficients(*coef)
        with pytest.raises(ValueError, match="^robin:.*required"):
            s.boundary_from(exact, grad=grad_exact)
        with pytest.raises(ValueError, match="^robin: shape"):
            s.set_coefficients(*coef, robin=np.zeros((6, n, n + 1)))
        with pytest.raises(ValueError, match="^robin: shape"):
            s.set_coefficients(*coef, robin=[1.0] * 5)
        with pytest.raises(ValueError, match="^robin: dtype"):
            s.set_coefficients(*coef, robin=kappa.astype(np.float32))
        with pytest.raises(ValueError, match="^robin:"):
            s.set_coefficients(*coef, robin="convective")
        for face, value, what in ((2, -1e-3, "out of range"), (3, np.nan, "not finite"), (0, np.inf, "not finite"), (5, np.nan, "not finite")):
            bad = kappa.copy()
            bad[face, 5, 7] = value                            # not finite: anywhere; negative: on a Robin face
            with pytest.raises(ValueError, match=f"^robin:.*{what}"):
                s.set_coefficients(*coef, robin=bad)
            with pytest.raises(ValueError):
                s.solve(f)                                     # no valid coefficients
        with pytest.raises(ValueError, match="^robin:.*out of range"):
            s.set_coefficients(*coef, robin=[0.0, 0.0, 1.0, -1.0, 0.0, 0.0])
        ok = kappa.copy()
        ok[0] = -3.0                                           # a Dirichlet face's entries are not read
        s.set_coefficients(*coef, robin=ok)
        u, info = s.solve(f)
        assert np.isfinite(u).all() and info.vcycles == 1
        p = [c.ctypes.data for c in coef[1:]]                  # the C entry points
        assert lib.hpgmg_user_set_coefficients(s._ptr, None, *p, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_set_coefficients_robin(s._ptr, None, *p, None, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_set_coefficients_robin(s._ptr, None, *p, kappa.ctypes.data, H.WHERE_HOST) == H.USER_OK
    for bc in ("dirichlet", ("neumann",) * 6):
        with Solver(n, box_dim=8, bc=bc, lib=lib) as s:
            with pytest.raises(ValueError, match="^robin:.*no 'convective' face"):
                s.set_coefficients(*coef, robin=kappa)
            with pytest.raises(ValueError, match="^robin:.*no 'convective' face"):
                s.boundary_from(exact, grad=grad_exact, robin=kappa)
            p = [c.ctypes.data for c in coef[1:]]
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, None, *p, kappa.ctypes.data, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, None, *p, None, H.WHERE_HOST) == H.USER_OK
    kinds = (ctypes.c_int * 6)(*[H.FACE_ROBIN] * 6)
    ptr = ctypes.c_void_p()
    assert lib.hpgmg_user_create_faces(n, 8, kinds, H.OP_7PT, H.SMOOTH_CHEBY, 0.0, 1.0, 0.0, ctypes.byref(ptr)) == H.USER_OK
    lib.hpgmg_user_destroy(ptr)
    for not_a_kind in (2, 4, -1):
        kinds[2] = not_a_kind
        assert lib.hpgmg_user_create_faces(n, 8, kinds, H.OP_7PT, H.SMOOTH_CHEBY, 0.0, 1.0, 0.0, ctypes.byref(ptr)) == H.USER_BAD_ARGUMENT

