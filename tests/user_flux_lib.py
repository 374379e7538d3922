"""Helpers of the face-flux tests (Solver.flux, Solver.wall_flux): the solvers the tests run on, an independent NumPy evaluation
of the fluxes from the dense arrays alone, and the rounding bounds derived from it.

The NumPy evaluation pads u with one ghost layer per wall -- 2 g - u on a Dirichlet wall, u + h gn on a Neumann wall, the Robin ghost
((2 - t) u + 2 h g) / (2 + t), t = kappa h, and the wrapped neighbour on a periodic box -- and then takes  q = (wq beta) (u_lo - u_hi)  on EVERY
face alike, with the wall's own beta on a wall.  The library never forms those ghosts: it evaluates the closed wall expressions of
include/hpgmg_boundary_math.h.  The two agree to rounding, not bitwise.
"""
import numpy as np

from user_robin_lib import ALL, CORNERS, D, N, R, kappa_of

EPS = np.finfo(np.float64).eps
NEUMANN_MIX = (N, D, N, N, D, N)         # Dirichlet i-high and k-low, the other four Neumann: N-N, N-D and D-D edges
# name -> bc= of the solver; "periodic" and "dirichlet" are the plain solvers
SOLVERS = {"dirichlet": "dirichlet", "periodic": "periodic", "corners": CORNERS, "robin": ALL, "neumann": NEUMANN_MIX}


def faces_of(name):
    bc = SOLVERS[name]
    return None if isinstance(bc, str) else bc


def kappa_for(name, n, h=None):
    """robin= of set_coefficients for that solver: the smooth kappa of user_robin_lib where a face is Robin, else None."""
    faces = faces_of(name)
    return kappa_of(n, faces, h) if faces is not None and R in faces else None


def boundary_for(name, n, seed):
    """Random data on every face (None for the periodic solver)."""
    return None if name == "periodic" else np.random.default_rng(seed).random((6, n, n)) * 4.0 - 2.0


def _along(a, axis):
    """View of a [k][j][i] array with axis i / j / k (0 / 1 / 2) first; the other two keep their order, which is that of a boundary face."""
    return np.moveaxis(a, 2 - axis, 0)


def padded(n, bc, faces, h, u, g, kappa, axis):
    """u with its two ghost layers along `axis` (first index 0 .. n+1), from the wall kinds and data alone."""
    U = _along(u, axis)
    P = np.empty((n + 2,) + U.shape[1:])
    P[1:-1] = U
    if bc == "periodic":
        P[0], P[-1] = U[-1], U[0]
        return P
    for side, cell, ghost in ((0, 1, 0), (1, n, n + 1)):
        face = 2 * axis + side
        gv = 0.0 if g is None else g[face]
        kind = D if faces is None else faces[face]
        if kind == D:
            P[ghost] = 2.0 * gv - P[cell]
        elif kind == N:
            P[ghost] = P[cell] + h * gv
        else:
            t = kappa[face] * h
            P[ghost] = ((2.0 - t) * P[cell] + 2.0 * h * gv) / (2.0 + t)
    return P


def reference(n, bc, faces, b, h, betas, u, g=None, kappa=None):
    """[(q, bound)] per axis in the shapes of the beta arrays: the NumPy fluxes and the elementwise bound  16 eps (wq beta) (|u_lo| + |u_hi| + 2 |g|)
    on what an evaluation of the same formulas in another order may differ by (|g| counts on wall faces only)."""
    wq = b * (1.0 / h)
    out = []
    for axis in range(3):
        P = padded(n, bc, faces, h, u, g, kappa, axis)
        B = _along(betas[axis], axis)
        lo, hi = (P[:-2], P[1:-1]) if bc == "periodic" else (P[:-1], P[1:])
        q = (wq * B) * (lo - hi)
        mag = np.abs(lo) + np.abs(hi)
        if bc != "periodic" and g is not None:
            mag[0] += 2.0 * np.abs(g[2 * axis])
            mag[-1] += 2.0 * np.abs(g[2 * axis + 1])
        bound = 16.0 * EPS * (wq * B) * mag
        out.append((np.ascontiguousarray(np.moveaxis(q, 0, 2 - axis)), np.ascontiguousarray(np.moveaxis(bound, 0, 2 - axis))))
    return out


def divergence(n, bc, h, fluxes):
    """(1/h) sum_d (q_d[high face] - q_d[low face]) per cell, (N,N,N)."""
    div = np.zeros((n, n, n))
    for axis, q in enumerate(fluxes):
        Q = _along(q, axis)
        high = np.roll(Q, -1, axis=0) if bc == "periodic" else Q[1:]
        low = Q if bc == "periodic" else Q[:-1]
        div += np.moveaxis(high - low, 0, 2 - axis)
    return div / h


def identity_bound(n, bc, a, h, alpha, u, bounds):
    """Per cell: 64 eps times the sum over the cell's six faces of (wq beta / h) (|u_lo| + |u_hi| + 2 |g|), plus 4 eps a alpha |u|; `bounds`
    are reference()'s, which hold 16 eps of the same face terms."""
    total = np.zeros((n, n, n))
    for axis, bnd in enumerate(bounds):
        Q = _along(bnd, axis)
        high = np.roll(Q, -1, axis=0) if bc == "periodic" else Q[1:]
        low = Q if bc == "periodic" else Q[:-1]
        total += np.moveaxis(high + low, 0, 2 - axis)
    total *= 4.0 / h
    if alpha is not None:
        total += 4.0 * EPS * a * alpha * np.abs(u)
    return total
