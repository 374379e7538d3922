"""Helpers of the Neumann / mixed-wall tests (Solver(n, bc=<6-tuple>)): the operator A_N and the lift T(g) with per-face kinds, the gradient of
the manufactured solution of user_boundary_lib, and F-cycle variants with parts of the level corrections left out.

Restates DESIGN.md §11.2: a wall cell's wall term is (b/h^2) beta_wall (u - u_ghost).  Dirichlet: u_ghost = 2 g - u, so the wall adds
2 (b/h^2) beta_wall to the diagonal and 2 (b/h^2) beta_wall g to the right-hand side.  Neumann: u_ghost = u + h gn (gn the outward normal
derivative), so the wall adds nothing to the matrix and (b/h) beta_wall gn to the right-hand side.
"""
import ctypes

import numpy as np

import hpgmg_amd as H
from user_problem_lib import assemble

ONE = ("dirichlet", "dirichlet", "dirichlet", "neumann", "dirichlet", "dirichlet")       # one Neumann face (j-high)
SIDES = ("dirichlet", "dirichlet", "neumann", "neumann", "neumann", "neumann")           # Dirichlet inlet / outlet, Neumann side walls
ALL = ("neumann",) * 6
CORNERS = ("neumann", "dirichlet", "dirichlet", "neumann", "neumann", "dirichlet")       # every corner and edge combination of the two kinds


def mask_of(faces):
    return sum(1 << f for f, kind in enumerate(faces) if kind == "neumann")


def wall_slices(n):
    """Index of face f's wall in (beta array number, index tuple): beta_i[:, :, 0], beta_i[:, :, n], beta_j[:, 0, :], ..."""
    s = slice(None)
    return [(0, (s, s, 0)), (0, (s, s, n)), (1, (s, 0, s)), (1, (s, n, s)), (2, (0, s, s)), (2, (n, s, s))]


def assemble_faces(n, faces, a, b, h, alpha, beta_i, beta_j, beta_k):
    """A_N as a SciPy matrix: a Neumann wall's term (b/h^2) beta (u - u) vanishes, which the Dirichlet assembly gives for a zero wall beta."""
    betas = [beta_i.copy(), beta_j.copy(), beta_k.copy()]
    for f, (which, idx) in enumerate(wall_slices(n)):
        if faces[f] == "neumann":
            betas[which][idx] = 0.0
    return assemble(n, "dirichlet", a, b, h, alpha, *betas)


def lift_faces(n, faces, b, h, beta_i, beta_j, beta_k, g):
    """T(g) on the (N,N,N) [k][j][i] grid: 2 b h^-2 beta g on a Dirichlet face, b h^-1 beta gn on a Neumann face."""
    betas = (beta_i, beta_j, beta_k)
    cells = [(slice(None), slice(None), 0), (slice(None), slice(None), -1), (slice(None), 0, slice(None)), (slice(None), -1, slice(None)),
             (0, slice(None), slice(None)), (-1, slice(None), slice(None))]
    T = np.zeros((n, n, n))
    for f, (which, idx) in enumerate(wall_slices(n)):
        c = b / h if faces[f] == "neumann" else 2.0 * b / (h * h)
        T[cells[f]] += c * betas[which][idx] * g[f]
    return T


def grad_exact(x, y, z):
    """grad of user_boundary_lib.exact: u* = sin(1.3x + 0.4) cos(0.7y - 0.2) exp(0.5z) + 0.3"""
    s, c = np.sin(1.3 * x + 0.4), np.cos(1.3 * x + 0.4)
    cy, sy, e = np.cos(0.7 * y - 0.2), np.sin(0.7 * y - 0.2), np.exp(0.5 * z)
    return 1.3 * c * cy * e, -0.7 * s * sy * e, 0.5 * s * cy * e


_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)


class _Hook(ctypes.Structure):      # hpgmg_fmg_hook of include/hpgmg_mg.h
    _fields_ = [("rhs_restricted", _CB), ("interpolated", _CB), ("ctx", ctypes.c_void_p), ("key", ctypes.c_longlong)]


def fcycle_variant(lib, s, f, g, coef, rhs_correction):
    """One F-cycle on f + T(g) of the oracle (its plugin memory is host memory) WITHOUT the interpolation correction, and with or without the
    right-hand-side correction (a) of DESIGN.md §11.1: the variants the public API cannot express, since a solver with a Neumann wall always
    runs with both.  Returns u."""
    n, b = s.n, s.b
    mask = mask_of(s.faces)
    s.set_rhs(f, boundary=g)                                   # F = f + T(g), mean shift included
    G = lib.hpgmg_solver_mg(lib.hpgmg_user_solver_of(s._ptr))
    levels = [lib.hpgmg_mg_level(G, l) for l in range(lib.hpgmg_mg_num_levels(G))]
    wall = np.zeros((6, n, n))
    for face, (which, idx) in enumerate(wall_slices(n)):
        wall[face] = coef[1 + which][idx]
    gs, walls, phis = [np.ascontiguousarray(g)], [wall], []
    for l, L in enumerate(levels):
        m = n >> l
        if l:
            for src in (gs, walls):
                dst = np.zeros((6, m, m))
                lib.hpgmg_boundary_restrict(L, dst.ctypes.data, levels[l - 1], src[-1].ctypes.data)
                src.append(dst)
        phi = np.zeros((6, m, m))
        assert lib.hpgmg_boundary_flux_faces(L, phi.ctypes.data, gs[l].ctypes.data, b, mask, walls[l].ctypes.data) == 0
        phis.append(phi)

    def restricted(hook, G_, l, R_id):
        if rhs_correction:
            lib.hpgmg_boundary_lift(levels[l], R_id, phis[l].ctypes.data, phis[l - 1].ctypes.data, 1.0)

    hook = _Hook(_CB(restricted), _CB(), None, 77)
    lib.hpgmg_fmg_set_hook.argtypes = [ctypes.c_void_p]
    lib.hpgmg_fmg_set_hook.restype = None
    lib.hpgmg_fmg_zero_u_first.restype = None
    lib.hpgmg_fmg_set_hook(ctypes.addressof(hook))
    try:
        lib.hpgmg_fmg_zero_u_first()
        lib.FMGSolve(G, 0, H.VECTOR_U, H.VECTOR_F, s.a, s.b, 1e-10)
    finally:
        lib.hpgmg_fmg_set_hook(None)
    return s.get_solution()
