"""Neumann and per-face mixed walls of the user-problem API (Solver(n, bc=<6-tuple> | "neumann"), hpgmg_user_create_faces) on the CPU oracle.

apply(x, boundary=g) is checked against a SciPy assembly of A_N x - T(g) and V-cycle solves against a direct solve; six
Dirichlet faces against bc="dirichlet" bit for bit; the packed betas level by level; the interpolation correction alone on a linear u; and on
a manufactured solution the order of the V-cycle error, the FMG property of the F-cycle and the V-cycle count next to Dirichlet walls.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_boundary_lib import exact, manufactured
from user_neumann_lib import ALL, CORNERS, ONE, SIDES, assemble_faces, fcycle_variant, grad_exact, lift_faces, mask_of, wall_slices
from user_problem_lib import random_coefficients

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8
WALLS = {"one": ONE, "sides": SIDES, "all": ALL}
# the project's FMG gate (test_oracle_user_boundary.py).  Measured on this oracle, one F-cycle's max error / the V-cycle solution's at
# N = 16, 32, 64: Neumann side walls 0.98, 0.98, 0.98; one Neumann face 0.90, 0.93, 0.95; six Neumann Helmholtz 1.01, 1.01, 1.01; six Neumann
# Poisson 1.20, 1.24, 1.26
FMG_FACTOR = 1.5
# the F-cycle without the interpolation correction, with or without (a): at least 34.8x (six Neumann Helmholtz, N = 16; every other entry of
# the table of DESIGN.md §11.2 is above 80x), growing about 4x per doubling
UNCORRECTED_FACTOR = 20.0
# second order predicts 4 per doubling; measured 3.70 - 4.00 (N = 16 .. 128)
ORDER_FACTOR = 3.0
# V-cycles to rtol 1e-10, measured on this oracle at N = 32 and 64 (the table of DESIGN.md §11.2): Chebyshev 9 with every wall set; GSRB 11 - 12
# with Dirichlet walls and at most 14 (Neumann side walls), Jacobi 10 - 11 and at most 12; six Neumann walls need fewer than Dirichlet.  The
# largest excess is 3 (GSRB, side walls, N = 32) and no count grows by more than one from N = 32 to 64, as the Dirichlet counts do.  The margin
# is that excess plus one.  (A first margin of 2, taken from the Chebyshev counts alone, did not hold for GSRB.)
VCYCLE_MARGIN = 4


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


def _random_boundary(n, seed):
    return np.random.default_rng(seed).random((6, n, n)) * 4.0 - 2.0


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
@pytest.mark.parametrize("walls", ["one", "sides", "all"])
def test_apply_matches_scipy_assembly(lib, walls, n, box_dim, a):
    faces = WALLS[walls]
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=100 + n + int(10 * a))
    b, h = 0.7, 1.0 / n
    x = np.random.default_rng(12).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 13)
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        y = s.apply(x, boundary=g)
        y0 = s.apply(x)
        yz = s.apply(x, boundary=np.zeros((6, n, n)))
    A = assemble_faces(n, faces, a, b, h, alpha, bi, bj, bk)
    ref = (A @ x.ravel()).reshape(n, n, n) - lift_faces(n, faces, b, h, bi, bj, bk, g)
    assert _rel(y, ref) <= 1e-13
    assert not np.array_equal(y, y0)
    assert np.array_equal(yz, y0)                              # boundary=None is zero data


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("walls,a", [("one", 0.0), ("one", 1.3), ("sides", 0.0), ("sides", 1.3), ("all", 1.3)])
def test_mg_solve_matches_direct_solve(lib, walls, n, box_dim, a):
    faces = WALLS[walls]
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=200 + n + int(10 * a))
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(7).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 8)
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        r = s.apply(u, boundary=g) - f
    assert info.converged and info.mean_shift == 0.0
    F = f + lift_faces(n, faces, b, h, bi, bj, bk, g)
    assert info.norm_f == pytest.approx(np.abs(F).max(), rel=1e-14)
    ref = spl.spsolve(assemble_faces(n, faces, a, b, h, alpha, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8
    assert np.abs(r).max() <= 1e-10 * np.abs(F).max()


@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_six_neumann_poisson_is_solved_up_to_its_mean(lib, n, box_dim):
    """Singular: the mean of f + T(g) is subtracted and reported; u agrees, mean removed, with a direct solve under the constraint mean(u) = 0."""
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=250 + n)
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(17).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 18)
    with Solver(n, box_dim=box_dim, bc="neumann", a=0.0, b=b, lib=lib) as s:
        assert s.faces == ALL
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        u_f, info_f = s.solve(f, method="fmg", boundary=g)
    F = f + lift_faces(n, ALL, b, h, bi, bj, bk, g)
    assert info.converged
    assert info.mean_shift == pytest.approx(F.mean(), rel=1e-12) and info_f.mean_shift == info.mean_shift
    A = assemble_faces(n, ALL, 0.0, b, h, None, bi, bj, bk)
    ones = np.ones((n ** 3, 1))
    K = sp.bmat([[A, sp.csr_matrix(ones)], [sp.csr_matrix(ones.T), None]]).tocsc()       # A u + lambda 1 = F, 1^T u = 0
    ref = spl.spsolve(K, np.concatenate([F.ravel(), [0.0]]))[:-1].reshape(n, n, n)
    assert _rel(u - u.mean(), ref - ref.mean()) <= 1e-8
    assert np.isfinite(u_f).all() and info_f.vcycles == 1


@pytest.mark.parametrize("smoother", ["cheby", "gsrb", "jacobi"])
@pytest.mark.parametrize("a", [0.0, 1.0])
def test_six_dirichlet_faces_are_the_dirichlet_solver(lib, smoother, a):
    n = 16
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=300 + len(smoother))
    f = np.random.default_rng(9).random((n, n, n)) - 0.4
    g = _random_boundary(n, 10)
    out = []
    for bc in ("dirichlet", ("dirichlet",) * 6):
        with Solver(n, box_dim=8, bc=bc, smoother=smoother, a=a, lib=lib) as s:
            assert s.faces is None
            s.set_coefficients(*coef)
            got = []
            for boundary in (None, g):
                for method in ("fmg", "mg"):
                    u, info = s.solve(f, method=method, boundary=boundary)
                    got += [u, np.array([info.residual, info.norm_f, info.vcycles])]
                    got.append(np.array(s.get_solution()))
                got.append(s.apply(f, boundary=boundary))
                L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0)
                F = np.empty((n, n, n))
                assert lib.hpgmg_dense_unpack(L, H.VECTOR_F, F.ctypes.data, H.WHERE_HOST) == 0
                got.append(F)
            out.append(got)
    assert len(out[0]) == len(out[1])
    for x, y in zip(*out):
        assert np.array_equal(x, y)
    kinds = (ctypes.c_int * 6)(*[H.FACE_DIRICHLET] * 6)          # the C entry point with six Dirichlet faces
    ptr = ctypes.c_void_p()
    assert lib.hpgmg_user_create_faces(n, 8, kinds, H.OP_7PT, H.SMOOTH_CHEBY, 0.0, 1.0, 0.0, ctypes.byref(ptr)) == H.USER_OK
    lib.hpgmg_user_destroy(ptr)
    kinds[2] = 2
    assert lib.hpgmg_user_create_faces(n, 8, kinds, H.OP_7PT, H.SMOOTH_CHEBY, 0.0, 1.0, 0.0, ctypes.byref(ptr)) == H.USER_BAD_ARGUMENT


def _level_vectors(lib, L, vid):
    info = (ctypes.c_int * H.INFO_COUNT)()
    lib.hpgmg_level_info(L, info)
    out = []
    for box in range(info[H.INFO_NUM_MY_BOXES]):
        low = (ctypes.c_int * 3)()
        lib.hpgmg_level_box_low(L, box, low)
        buf = np.empty(info[H.INFO_VOLUME])
        lib.hpgmg_level_read_vector(L, box, vid, buf.ctypes.data)
        out.append((tuple(low), buf))
    return info, out


@pytest.mark.parametrize("walls", ["one", "sides", "all"])
@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_level_beta_is_zero_on_neumann_walls_only(lib, walls, n, box_dim):
    """Every level: the beta vectors are 0.0 on the Neumann walls and, everywhere else, what the all-Dirichlet solver holds."""
    faces = WALLS[walls]
    coef = random_coefficients(n, "dirichlet", True, seed=350 + n)
    with Solver(n, box_dim=box_dim, bc=faces, a=1.0, lib=lib) as s, Solver(n, box_dim=box_dim, a=1.0, lib=lib) as d:
        s.set_coefficients(*coef)
        d.set_coefficients(*coef)
        Gs, Gd = (lib.hpgmg_solver_mg(lib.hpgmg_user_solver_of(x._ptr)) for x in (s, d))
        levels = min(lib.hpgmg_mg_num_levels(Gs), lib.hpgmg_mg_num_levels(Gd))
        assert levels >= 3
        walls_seen = 0
        for l in range(levels):
            Ls, Ld = lib.hpgmg_mg_level(Gs, l), lib.hpgmg_mg_level(Gd, l)
            for axis, vid in enumerate((H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)):
                info, got = _level_vectors(lib, Ls, vid)
                _, ref = _level_vectors(lib, Ld, vid)
                nl, dim, gh = info[H.INFO_DIM], info[H.INFO_BOX_DIM], info[H.INFO_GHOSTS]
                jS, kS = info[H.INFO_JSTRIDE], info[H.INFO_KSTRIDE]
                for (low, v), (low_d, vd) in zip(got, ref):
                    assert low == low_d
                    # the cells the operator reads: interior indices 0 .. dim along the array's axis (dim: the high face), 0 .. dim-1 across
                    idx = np.arange(dim + 1)[:, None, None] * (1, jS, kS)[axis]
                    across = [x for x in range(3) if x != axis]
                    idx = idx + np.arange(dim)[None, :, None] * (1, jS, kS)[across[0]] + np.arange(dim)[None, None, :] * (1, jS, kS)[across[1]]
                    idx = idx + gh * (1 + jS + kS)
                    a_s, a_d = v[idx], vd[idx]
                    expect = a_d.copy()
                    if faces[2 * axis] == "neumann" and low[axis] == 0:
                        expect[0] = 0.0
                        walls_seen += 1
                    if faces[2 * axis + 1] == "neumann" and low[axis] + dim == nl:
                        expect[dim] = 0.0
                        walls_seen += 1
                    assert (a_d > 0.0).all()
                    assert np.array_equal(a_s, expect), (l, axis, low)
        assert walls_seen >= levels * mask_of(faces).bit_count()


def _linear(x, y, z):
    return 0.3 + 1.1 * x - 0.7 * y + 0.5 * z


def _linear_grad(x, y, z):
    return 1.1 + 0.0 * x, -0.7 + 0.0 * x, 0.5 + 0.0 * x


@pytest.mark.parametrize("walls", [ONE, SIDES, ALL, CORNERS], ids=["one", "sides", "all", "corners"])
def test_interpolation_correction_reproduces_a_linear_function(lib, walls):
    """interpolation_fcycle (p1) from level l+1 plus the hook's correction gives a linear u exactly on level l, boundary cells included."""
    n = 16
    with Solver(n, box_dim=8, bc=walls, lib=lib) as s:
        G = lib.hpgmg_solver_mg(lib.hpgmg_user_solver_of(s._ptr))
        for l in (0, 1):
            Lf, Lc = lib.hpgmg_mg_level(G, l), lib.hpgmg_mg_level(G, l + 1)
            nf, nc = n >> l, n >> (l + 1)
            assert lib.hpgmg_level_h(Lc) == pytest.approx(1.0 / nc)
            cf, cc = (np.arange(nf) + 0.5) / nf, (np.arange(nc) + 0.5) / nc
            Z, Y, X = np.meshgrid(cc, cc, cc, indexing="ij")
            uc = np.ascontiguousarray(_linear(X, Y, Z))
            with Solver(nc, box_dim=4, bc=walls, h=1.0 / nc, lib=lib) as sampler:       # the coarse level's face centres
                gc = sampler.boundary_from(_linear, grad=_linear_grad)
            zero = np.zeros((nf, nf, nf))
            assert lib.hpgmg_dense_pack(Lc, H.VECTOR_U, uc.ctypes.data, H.WHERE_HOST, 0, 0) == 0
            assert lib.hpgmg_dense_pack(Lf, H.VECTOR_U, zero.ctypes.data, H.WHERE_HOST, 0, 0) == 0
            lib.interpolation_fcycle(Lf, H.VECTOR_U, 0.0, Lc, H.VECTOR_U)
            plain = np.empty((nf, nf, nf))
            assert lib.hpgmg_dense_unpack(Lf, H.VECTOR_U, plain.ctypes.data, H.WHERE_HOST) == 0
            lib.hpgmg_boundary_interp_faces(Lf, H.VECTOR_U, Lc, gc.ctypes.data, mask_of(walls))
            got = np.empty((nf, nf, nf))
            assert lib.hpgmg_dense_unpack(Lf, H.VECTOR_U, got.ctypes.data, H.WHERE_HOST) == 0
            Z, Y, X = np.meshgrid(cf, cf, cf, indexing="ij")
            ref = _linear(X, Y, Z)
            assert np.abs(got - ref).max() <= 1e-14, (l, np.abs(got - ref).max())
            shell = np.ones_like(ref, dtype=bool)
            shell[1:-1, 1:-1, 1:-1] = False
            assert np.array_equal(got[~shell], plain[~shell])                # only boundary cells are touched
            assert np.abs(plain - ref)[shell].max() > 0.1                      # which the homogeneous ghosts leave far off


def _errors(lib, n, a, faces, variants=False):
    coef = manufactured(n, a, 1.0)
    alpha, bi, bj, bk, f, u_star = coef
    free = faces == ALL and a == 0.0

    def err(u):
        return np.abs((u - u.mean()) - (u_star - u_star.mean())).max() if free else np.abs(u - u_star).max()

    with Solver(n, box_dim=min(n // 2, 32), bc=faces, a=a, b=1.0, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        g = s.boundary_from(exact, grad=grad_exact)
        assert np.all(np.abs(g) > 1e-3)                        # non-zero data on every face
        u_mg, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        u_fmg, info_f = s.solve(f, method="fmg", boundary=g)
        assert info.converged and info_f.vcycles == 1
        out = [err(u_mg), err(u_fmg)]
        if variants:
            out += [err(fcycle_variant(lib, s, f, g, coef, True)), err(fcycle_variant(lib, s, f, g, coef, False))]
    return out


@pytest.mark.parametrize("walls,a", [("sides", 1.0), ("sides", 0.0), ("all", 1.0), ("all", 0.0)])
def test_manufactured_solution_is_second_order(lib, walls, a):
    errs = [_errors(lib, n, a, WALLS[walls])[0] for n in (16, 32, 64, 128)]
    factors = [errs[i] / errs[i + 1] for i in range(3)]
    print(f"{walls} a={a}: V-cycle errors {errs}, factors {factors}")
    assert min(factors) >= ORDER_FACTOR, (errs, factors)


@pytest.mark.parametrize("walls,a", [("sides", 1.0), ("sides", 0.0), ("one", 1.0), ("all", 1.0), ("all", 0.0)])
def test_one_fcycle_is_as_accurate_as_vcycles(lib, walls, a):
    """With both level corrections; without the interpolation correction (with (a) only, and with neither) far outside the gate."""
    for n in (16, 32, 64):
        e_mg, e_fmg, e_rhs_only, e_neither = _errors(lib, n, a, WALLS[walls], variants=True)
        print(f"{walls} a={a} N={n}: V-cycles {e_mg:.3e}; F-cycle {e_fmg / e_mg:.3f}x, without (b) {e_rhs_only / e_mg:.1f}x, with neither {e_neither / e_mg:.1f}x")
        assert e_fmg <= FMG_FACTOR * e_mg, (n, e_fmg, e_mg)
        assert e_rhs_only >= UNCORRECTED_FACTOR * e_mg, (n, e_rhs_only, e_mg)
        assert e_neither >= UNCORRECTED_FACTOR * e_mg, (n, e_neither, e_mg)


@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("smoother", ["cheby", "gsrb", "jacobi"])
@pytest.mark.parametrize("a", [0.0, 1.0])
def test_vcycle_count_next_to_dirichlet_walls(lib, smoother, a, n):
    alpha, bi, bj, bk, f, _ = manufactured(n, a, 1.0)
    counts = {}
    for name, faces in (("dirichlet", "dirichlet"), ("one", ONE), ("sides", SIDES), ("corners", CORNERS), ("all", ALL)):
        with Solver(n, box_dim=16, bc=faces, smoother=smoother, a=a, b=1.0, lib=lib) as s:
            s.set_coefficients(alpha, bi, bj, bk)
            g = s.boundary_from(exact, grad=grad_exact)
            _, info = s.solve(f, method="mg", rtol=1e-10, boundary=g)
            assert info.converged
            counts[name] = info.vcycles
    print(f"N={n} {smoother} a={a}: V-cycles to 1e-10 {counts}")
    for name in ("one", "sides", "corners", "all"):
        assert counts[name] <= counts["dirichlet"] + VCYCLE_MARGIN, counts


def test_boundary_from_samples_the_outward_normal_derivative(lib):
    n = 8
    with Solver(n, box_dim=4, bc=CORNERS, h=0.5, lib=lib) as s:
        g = s.boundary_from(lambda x, y, z: x + 10.0 * y + 100.0 * z, grad=lambda x, y, z: (1.0 + 0 * x, 10.0 + 0 * x, 100.0 + 0 * x))
    c = (np.arange(n) + 0.5) * 0.5
    assert np.array_equal(g[0], np.full((n, n), -1.0))                              # i-low, Neumann: -du/dx
    assert np.array_equal(g[1], n * 0.5 + 10.0 * c[None, :] + 100.0 * c[:, None])   # i-high, Dirichlet: u
    assert np.array_equal(g[3], np.full((n, n), 10.0))                              # j-high, Neumann: +du/dy
    assert np.array_equal(g[4], np.full((n, n), -100.0))                            # k-low, Neumann: -du/dz


def test_refusals(lib):
    n = 16
    with pytest.raises(ValueError, match="^bc:.*6 entries"):
        Solver(n, box_dim=8, bc=("neumann",) * 5, lib=lib)
    with pytest.raises(ValueError, match="^bc:.*'robin'"):
        Solver(n, box_dim=8, bc=("neumann", "robin") + ("dirichlet",) * 4, lib=lib)
    with pytest.raises(ValueError, match="^bc:.*periodic"):
        Solver(n, box_dim=8, bc=("periodic", "periodic") + ("neumann",) * 4, lib=lib)
    with pytest.raises(ValueError, match="^bc:"):
        Solver(n, box_dim=8, bc="robin", lib=lib)
    coef = random_coefficients(n, "dirichlet", False, seed=400)
    f = np.ones((n, n, n))
    g = _random_boundary(n, 14)
    with Solver(n, box_dim=8, bc=SIDES, lib=lib) as s:
        with pytest.raises(ValueError, match="^grad:"):
            s.boundary_from(exact)
        s.set_coefficients(None, *coef[1:])
        bad = g.copy(); bad[3, 15, 15] = np.nan                # a Neumann face's entry
        with pytest.raises(ValueError, match="^boundary:.*not finite"):
            s.solve(f, boundary=bad)
        with pytest.raises(ValueError, match="^boundary:.*not finite"):
            s.apply(f, boundary=bad)
        with pytest.raises(ValueError, match="^boundary: shape"):
            s.solve(f, boundary=np.zeros((6, n, n + 1)))
        for wall, name in (((slice(None), 0, slice(None)), "beta_j"), ((n, slice(None), slice(None)), "beta_k")):
            betas = {"beta_i": coef[1], "beta_j": coef[2].copy(), "beta_k": coef[3].copy()}
            betas[name][wall][3, 5] = 0.0                      # a Neumann wall's beta is still validated
            with pytest.raises(ValueError, match=f"^{name}:.*out of range"):
                s.set_coefficients(None, betas["beta_i"], betas["beta_j"], betas["beta_k"])
            with pytest.raises(ValueError):
                s.solve(f, boundary=g)                         # no valid coefficients
        s.set_coefficients(None, *coef[1:])
        u, info = s.solve(f, boundary=g)                       # still usable
        assert np.isfinite(u).all() and info.vcycles == 1
    with Solver(n, box_dim=8, bc="dirichlet", lib=lib) as s:   # a Dirichlet solver samples values as before, grad not needed
        assert s.boundary_from(exact).shape == (6, n, n)
