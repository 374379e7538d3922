"""Cell-centred conductivities (Solver.set_cell_coefficients, Solver.cell_sensitivity; hpgmg_user_set_cell_coefficients, hpgmg_user_cell_sensitivity;
the hooks hpgmg_dense_pack_cell_mean, hpgmg_dense_unpack_cell_sensitivity) on the CPU oracle.  DESIGN.md §11.10.

set_cell_coefficients(alpha, k, mean) must be set_coefficients(alpha, *face_mean(k)) bit for bit, and cell_sensitivity the existing sensitivity pass
followed by the gather of user_cells_lib (the restatement of the chain rule).  The restatement's transpose is checked by itself, in NumPy, against
central differences of the face mean.  Then the statuses, by name, and what the calls leave untouched.
"""
import math

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_cells_lib import MEANS, STATUS_CASES, block_field, cell_gather, cell_terms, face_mean, planted
from user_flux_lib import EPS, SOLVERS, boundary_for, kappa_for

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8: boxes on zero to three walls, box-to-box and periodic-wrap faces
NAMES = ["dirichlet", "periodic", "corners", "robin", "neumann"]
A, B = 1.3, 0.7


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _bc_name(name):
    return "periodic" if name == "periodic" else "dirichlet"


def _problem(name, n, a, seed):
    rng = np.random.default_rng(seed + 1)
    alpha = rng.random((n, n, n)) + 0.5 if a != 0.0 else None
    x, lam = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 2.0 - 1.0
    return _bc_name(name), alpha, block_field(n, seed), x, lam, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _bytes(q):
    return [None if x is None else x.tobytes() for x in q]


# ---------------------------------------------------------------- 1. the same bytes as the face route
@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, A])
@pytest.mark.parametrize("name", NAMES)
def test_same_bytes_as_the_face_route(lib, name, a, n, box_dim, mean):
    """apply, flux (a Neumann or Robin wall's own beta weighs its data) and an "mg" solve of the two solvers are identical as 64-bit patterns."""
    bc, alpha, k, x, _, g, kappa = _problem(name, n, a, 3000 + n + int(10 * a))
    f = np.random.default_rng(3001).random((n, n, n)) - 0.5
    with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B, lib=lib) as s, Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B, lib=lib) as t:
        s.set_cell_coefficients(alpha, k, mean=mean, robin=kappa)
        t.set_coefficients(alpha, *face_mean(n, bc, k, mean), robin=kappa)
        assert s.apply(x, boundary=g).tobytes() == t.apply(x, boundary=g).tobytes()
        assert _bytes(s.flux(x, boundary=g)) == _bytes(t.flux(x, boundary=g))
        (u, info), (v, _) = s.solve(f, method="mg", boundary=g), t.solve(f, method="mg", boundary=g)
        assert u.tobytes() == v.tobytes() and np.isfinite(u).all() and info.vcycles > 0


# ---------------------------------------------------------------- 2. cell_sensitivity
@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, A])
@pytest.mark.parametrize("name", NAMES)
def test_cell_sensitivity_is_the_pass_plus_the_gather(lib, name, a, n, box_dim, mean):
    """d_alpha has sensitivity's bytes, d_k those of cell_gather(k, *sensitivity(u, lam, boundary=g)[1:]); every entry written over a NaN pre-fill."""
    bc, alpha, k, u, lam, g, kappa = _problem(name, n, a, 3100 + n + int(10 * a))
    with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B, lib=lib) as s:
        s.set_cell_coefficients(alpha, k, mean=mean, robin=kappa)
        G = s.sensitivity(u, lam, boundary=g)
        into = (np.full((n, n, n), np.nan) if a != 0.0 else None, np.full((n, n, n), np.nan))
        got = s.cell_sensitivity(u, lam, k, mean=mean, boundary=g, out=into)
        assert got[0] is into[0] and got[1] is into[1]
        assert _bytes(s.cell_sensitivity(u, lam, k, mean=mean, boundary=g)) == _bytes(into)
    assert (got[0] is None) == (a == 0.0)
    assert _bytes([got[0]]) == _bytes([G[0]])
    assert np.isfinite(got[1]).all()
    assert got[1].tobytes() == cell_gather(n, bc, k, mean, *G[1:]).tobytes()


# ---------------------------------------------------------------- 3. the restatement's transpose (pure NumPy)
def _dot_faces(G, F):
    return math.fsum(np.concatenate([(x * y).ravel() for x, y in zip(G, F)]))


@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("n", [16, 24])
def test_the_gather_is_the_transpose_of_the_harmonic_mean(bc, n):
    """sum_c cell_gather(k, G)_c d_c against the central difference of sum_f G_f face_mean(k +- eps d)_f at eps = 0.2, 0.1, 0.05: d has entries in
    (-1/2, 1/2), so k +- eps d >= 0.4.  The harmonic mean is smooth there, so the central difference misses by O(eps^2): successive misses fall by a
    ratio in [3.5, 4.5], the gate of DESIGN.md §11.9 (4.00 to 4.06 measured)."""
    rng = np.random.default_rng(3200 + n)
    k = block_field(n, 3201 + n)
    d = rng.random((n, n, n)) - 0.5
    G = [rng.random(F.shape) * 2.0 - 1.0 for F in face_mean(n, bc, k, "harmonic")]
    value = math.fsum((cell_gather(n, bc, k, "harmonic", *G) * d).ravel())
    misses = []
    for eps in (0.2, 0.1, 0.05):
        up, down = face_mean(n, bc, k + eps * d, "harmonic"), face_mean(n, bc, k - eps * d, "harmonic")
        misses.append(abs((_dot_faces(G, up) - _dot_faces(G, down)) / (2.0 * eps) - value))
    ratios = [misses[0] / misses[1], misses[1] / misses[2]]
    print(f"{bc} N={n}: value = {value:.12e}, misses / |value| = {[m / abs(value) for m in misses]}, ratios = {ratios}")
    assert all(3.5 <= r <= 4.5 for r in ratios), (misses, ratios)


@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("n", [16, 24])
def test_the_gather_is_the_transpose_of_the_arithmetic_mean(bc, n):
    """The arithmetic mean is linear in k, so one increment is exact: sum_c cell_gather(k, G)_c d_c = sum_f G_f face_mean(d)_f to rounding.  The bound
    is 8 eps sum |G| |mean factor| |d| -- six products and a six-term sum per cell on one side, a product, a sum and a product per face on the other."""
    rng = np.random.default_rng(3300 + n)
    k = block_field(n, 3301 + n)
    d = rng.random((n, n, n)) - 0.5
    G = [rng.random(F.shape) * 2.0 - 1.0 for F in face_mean(n, bc, k, "arithmetic")]
    lhs = math.fsum((cell_gather(n, bc, k, "arithmetic", *G) * d).ravel())
    rhs = _dot_faces(G, face_mean(n, bc, d, "arithmetic"))
    terms, factors = cell_terms(n, bc, k, "arithmetic", *[np.abs(x) for x in G])
    bound = 8.0 * EPS * math.fsum(np.concatenate([(t * np.abs(d)).ravel() for t in terms]))
    assert all(((D == 0.5) | (D == 1.0)).all() for D in factors)
    print(f"{bc} N={n}: lhs = {lhs:.15e}, rhs = {rhs:.15e}, |difference| = {abs(lhs - rhs):.3e} = {abs(lhs - rhs) / bound:.3f} of the bound")
    assert abs(lhs - rhs) <= bound


# ---------------------------------------------------------------- 4. statuses, from host arrays
@pytest.mark.parametrize("case", STATUS_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("name", ["dirichlet", "periodic", "corners"])
def test_statuses(lib, name, case):
    """The status of the C call, the ValueError that names k, and a refused call leaves the solver NOT_READY as a refused set_coefficients does.
    cell_sensitivity validates k the same way."""
    _, plants, mean, status, says = case
    n = 24
    _, alpha, good, u, lam, g, kappa = _problem(name, n, 0.0, 3400)
    k = planted(n, plants)
    m = H.MEAN_HARMONIC if mean == "harmonic" else H.MEAN_ARITHMETIC
    pk = None if kappa is None else kappa.ctypes.data
    with Solver(n, box_dim=8, bc=SOLVERS[name], b=B, lib=lib) as s:
        assert lib.hpgmg_user_set_cell_coefficients(s._ptr, None, k.ctypes.data, m, pk, H.WHERE_HOST) == status
        assert lib.hpgmg_user_apply(s._ptr, u.ctypes.data, lam.ctypes.data, H.WHERE_HOST) == H.USER_NOT_READY
        with pytest.raises(ValueError, match=f"^k:.*{says}"):
            s.set_cell_coefficients(None, k, mean=mean, robin=kappa)
        s.set_cell_coefficients(None, good, mean=mean, robin=kappa)
        out = np.empty((n, n, n))
        assert lib.hpgmg_user_cell_sensitivity(s._ptr, u.ctypes.data, lam.ctypes.data, k.ctypes.data, m, None, None, out.ctypes.data, H.WHERE_HOST) == status
        with pytest.raises(ValueError, match=f"^k:.*{says}"):
            s.cell_sensitivity(u, lam, k, mean=mean, boundary=g)


def test_the_arithmetic_mean_takes_what_overflows_the_harmonic_product(lib):
    n = 16
    k = planted(n, [((3, 4, 5), 1e200), ((3, 4, 6), 1e200)])
    with Solver(n, box_dim=8, lib=lib) as s:
        s.set_cell_coefficients(None, k, mean="arithmetic")


def test_refusals_by_name(lib):
    n = 16
    _, alpha, k, u, lam, g, _ = _problem("dirichlet", n, A, 3500)
    with Solver(n, box_dim=8, a=A, b=B, lib=lib) as s:
        with pytest.raises(ValueError, match="^alpha: required"):
            s.set_cell_coefficients(None, k)
        with pytest.raises(ValueError, match="^mean:.*'geometric'"):
            s.set_cell_coefficients(alpha, k, mean="geometric")
        with pytest.raises(ValueError, match="^robin: this solver has no"):
            s.set_cell_coefficients(alpha, k, robin=np.zeros((6, n, n)))
        with pytest.raises(ValueError, match="^k: shape"):
            s.set_cell_coefficients(alpha, face_mean(n, "dirichlet", k, "harmonic")[0])
        with pytest.raises(ValueError, match="^k: dtype"):
            s.set_cell_coefficients(alpha, k.astype(np.float32))
        with pytest.raises(ValueError, match="^k: expected"):
            s.set_cell_coefficients(alpha, k.tolist())
        with pytest.raises(ValueError, match="^alpha: shape"):
            s.set_cell_coefficients(alpha[:-1], k)
        bad = alpha.copy()
        bad[1, 2, 3] = -1.0
        with pytest.raises(ValueError, match="^alpha:.*out of range"):
            s.set_cell_coefficients(bad, k)
        with pytest.raises(ValueError, match="^u, lam, k, boundary: no valid coefficients"):
            s.cell_sensitivity(u, lam, k, boundary=g)
        s.set_cell_coefficients(alpha, k)
        good = s.cell_sensitivity(u, lam, k, boundary=g)
        with pytest.raises(ValueError, match="^mean:"):
            s.cell_sensitivity(u, lam, k, mean=1)
        with pytest.raises(ValueError, match="^k: shape"):
            s.cell_sensitivity(u, lam, k[:-1])
        with pytest.raises(ValueError, match="^lam: shape"):
            s.cell_sensitivity(u, lam[:-1], k)
        with pytest.raises(ValueError, match="^out: expected a pair"):
            s.cell_sensitivity(u, lam, k, out=good[1])
        with pytest.raises(ValueError, match="^out: expected a pair"):
            s.cell_sensitivity(u, lam, k, out=good + good)
        with pytest.raises(ValueError, match=r"^out\[0\]"):
            s.cell_sensitivity(u, lam, k, out=(None, good[1]))
        with pytest.raises(ValueError, match=r"^out\[1\]: dtype"):
            s.cell_sensitivity(u, lam, k, out=(good[0], good[1].astype(np.float32)))
        with pytest.raises(ValueError, match=r"^out\[1\]"):
            s.cell_sensitivity(u, lam, k, out=(good[0], None))
        bad = u.copy()
        bad[3, 4, 5] = np.inf
        with pytest.raises(ValueError, match="^u:.*not finite"):
            s.cell_sensitivity(bad, lam, k, boundary=g)
        bad_g = g.copy()
        bad_g[5, n - 1, 0] = np.nan
        with pytest.raises(ValueError, match="^boundary:.*not finite"):
            s.cell_sensitivity(u, lam, k, boundary=bad_g)
        call = lib.hpgmg_user_cell_sensitivity
        p = [x.ctypes.data for x in (u, lam, k)]
        raw = [np.empty((n, n, n)), np.empty((n, n, n))]
        o = [x.ctypes.data for x in raw]
        assert call(s._ptr, *p, H.MEAN_HARMONIC, None, *o, H.WHERE_HOST) == H.USER_OK
        assert call(s._ptr, p[0], p[1], None, H.MEAN_HARMONIC, None, *o, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, *p, H.MEAN_HARMONIC, None, o[0], None, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, *p, H.MEAN_HARMONIC, None, None, o[1], H.WHERE_HOST) == H.USER_BAD_ARGUMENT      # no d_alpha with a != 0
        assert call(s._ptr, *p, 2, None, *o, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, *p, H.MEAN_HARMONIC, None, *o, 2) == H.USER_BAD_ARGUMENT
        set_ = lib.hpgmg_user_set_cell_coefficients
        assert set_(s._ptr, alpha.ctypes.data, None, H.MEAN_HARMONIC, None, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert set_(s._ptr, alpha.ctypes.data, p[2], -1, None, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert set_(s._ptr, None, p[2], H.MEAN_HARMONIC, None, H.WHERE_HOST) == H.USER_BAD_ARGUMENT             # no alpha with a != 0
        assert set_(s._ptr, alpha.ctypes.data, p[2], H.MEAN_HARMONIC, g.ctypes.data, H.WHERE_HOST) == H.USER_BAD_ARGUMENT      # kappa without a Robin face
        assert _bytes(s.cell_sensitivity(u, lam, k, boundary=g)) == _bytes(good)                              # none of them disturbed the solver
    with Solver(n, box_dim=8, bc=SOLVERS["robin"], lib=lib) as s:
        with pytest.raises(ValueError, match="^robin: required"):
            s.set_cell_coefficients(None, k)
        kap = np.full((6, n, n), -1.0)
        with pytest.raises(ValueError, match="^robin:.*out of range"):
            s.set_cell_coefficients(None, k, robin=kap)
        s.set_cell_coefficients(None, k, robin=(0.5,) * 6)
    with Solver(n, box_dim=8, bc="periodic", lib=lib) as s:
        s.set_cell_coefficients(None, k)
        with pytest.raises(ValueError, match="^boundary:.*Dirichlet"):
            s.cell_sensitivity(u, lam, k, boundary=g)


# ---------------------------------------------------------------- 5. the hooks' refusals: -1 and nothing written
def test_the_hooks_refuse_with_nothing_written(lib):
    n = 16
    k = block_field(n, 3600)
    with Solver(n, box_dim=8, a=A, b=B, lib=lib) as s, Solver(n, box_dim=8, bc="periodic", a=A, b=B, lib=lib) as per:
        L, Lp = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0), lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(per._ptr), 0)
        x = np.random.default_rng(3601).random((n, n, n))
        before = s.apply(x).tobytes()
        wall = lib.hpgmg_vector_alloc(6 * n * n)
        pack, P = lib.hpgmg_dense_pack_cell_mean, k.ctypes.data
        try:
            assert pack(L, None, H.WHERE_HOST, H.MEAN_HARMONIC, 0, None) == -1
            assert pack(L, P, 2, H.MEAN_HARMONIC, 0, None) == -1
            assert pack(L, P, H.WHERE_HOST, 2, 0, None) == -1
            assert pack(L, P, H.WHERE_HOST, H.MEAN_HARMONIC, 64, wall) == -1
            assert pack(L, P, H.WHERE_HOST, H.MEAN_HARMONIC, -1, wall) == -1
            assert pack(L, P, H.WHERE_HOST, H.MEAN_HARMONIC, 5, None) == -1             # a mask without wall
            assert pack(Lp, P, H.WHERE_HOST, H.MEAN_HARMONIC, 5, wall) == -1            # a mask on a periodic level
        finally:
            lib.hpgmg_vector_free(wall)
        assert s.apply(x).tobytes() == before                                          # the coefficient vectors are as they were
        out = np.full((n, n, n), np.nan)
        sens = lib.hpgmg_dense_unpack_cell_sensitivity
        u_id, l_id = H.VECTOR_U, H.VECTOR_F
        assert sens(L, u_id, l_id, None, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, out.ctypes.data, H.WHERE_HOST) == -1
        assert sens(L, u_id, l_id, P, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, None, H.WHERE_HOST) == -1
        assert sens(L, u_id, l_id, P, 7, None, A, B, 0, None, None, None, out.ctypes.data, H.WHERE_HOST) == -1
        assert sens(L, -1, l_id, P, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, out.ctypes.data, H.WHERE_HOST) == -1
        assert sens(L, u_id, l_id, P, H.MEAN_HARMONIC, None, A, B, 5, None, None, None, out.ctypes.data, H.WHERE_HOST) == -1
        assert sens(L, u_id, l_id, P, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, out.ctypes.data, 2) == -1
        assert np.isnan(out).all()


# ---------------------------------------------------------------- 6. lifecycle
def test_the_coefficient_version_counts_set_cell_coefficients(lib):
    n = 16
    _, alpha, k, _, _, _, _ = _problem("dirichlet", n, A, 3700)
    with Solver(n, box_dim=8, a=A, lib=lib) as s:
        v0 = s.coefficient_version
        s.set_cell_coefficients(alpha, k)
        v1 = s.coefficient_version
        s.set_cell_coefficients(alpha, k, mean="arithmetic")
        assert v0 < v1 < s.coefficient_version


def test_set_cell_coefficients_ends_a_march(lib):
    n = 16
    _, alpha, k, u0, _, g, _ = _problem("dirichlet", n, A, 3710)
    f = np.random.default_rng(3711).random((n, n, n)) - 0.5
    with Solver(n, box_dim=8, a=A, lib=lib) as s:
        s.set_cell_coefficients(alpha, k)
        s.start(u0, f, boundary=g, dt=1e-3)
        s.step(f, boundary=g)
        s.set_cell_coefficients(alpha, k)
        with pytest.raises(ValueError, match="^step: no march is live"):
            s.step(f, boundary=g)


@pytest.mark.parametrize("name", ["dirichlet", "periodic", "corners"])
def test_cell_sensitivity_leaves_the_solver_as_it_was(lib, name):
    import ctypes
    n = 16
    _, alpha, k, x, lam, g, kappa = _problem(name, n, A, 3720)
    f = np.random.default_rng(3721).random((n, n, n)) - 0.5
    with Solver(n, box_dim=8, bc=SOLVERS[name], a=A, lib=lib) as s:
        s.set_cell_coefficients(alpha, k, robin=kappa)
        u, _ = s.solve(f, boundary=g)
        again, _ = s.solve(f, method="mg", boundary=g)          # what a second solve gives without a call in between
        u, _ = s.solve(f, boundary=g)
        s.cell_sensitivity(x, lam, k, boundary=None if g is None else -g)      # other operands, other data
        assert s.get_solution().tobytes() == u.tobytes()
        info = H.UserInfo()                                     # the right-hand side of the last set_rhs is still in place
        assert lib.hpgmg_user_solve(s._ptr, H.USER_MG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_OK
        assert s.get_solution().tobytes() == again.tobytes()


@pytest.mark.parametrize("name", ["dirichlet", "corners"])
def test_a_march_survives_cell_sensitivity(lib, name):
    """The bytes of the next step are those of an undisturbed march."""
    n = 16
    _, alpha, k, x, lam, g, kappa = _problem(name, n, A, 3730)
    rng = np.random.default_rng(3731)
    u0, f = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5
    seen = []
    for disturb in (False, True):
        with Solver(n, box_dim=8, bc=SOLVERS[name], a=A, lib=lib) as s:
            s.set_cell_coefficients(alpha, k, robin=kappa)
            s.start(u0, f, boundary=g, dt=1e-3, theta=0.5)
            s.step(f, boundary=g)
            if disturb:
                s.cell_sensitivity(x, lam, k, boundary=-g)
            info = s.step(f, boundary=g)
            seen.append((s.get_solution().tobytes(), s.rate().tobytes(), info.rate, info.residual))
    assert seen[0] == seen[1]
