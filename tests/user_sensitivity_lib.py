"""Helpers of the sensitivity tests (Solver.sensitivity, hpgmg_amd.autograd): a NumPy restatement of the table of §11.9 from
the dense arrays alone, with the rounding bounds of an evaluation in another order, and the sums the linearity identity compares.

The restatement writes every expression in the operation order of include/hpgmg_boundary_math.h (bnd_sens_*).  NumPy evaluates one IEEE
operation per call and every build of the library has -ffp-contract=off, so the restatement does not only agree within the bound: it has the
library's bits, and the GPU tests compare it bitwise.  It shares no code with the library: slices of the dense arrays, not boxes.
"""
import math

import numpy as np

from user_flux_lib import EPS, _along
from user_robin_lib import D, R


def restatement(n, bc, faces, a, b, h, u, lam, g=None, kappa=None):
    """[(G, bound)] for d_alpha, d_beta_i, d_beta_j, d_beta_k (the first is (None, None) when a == 0): G in the shapes of the coefficient
    arrays, and the elementwise bound  16 eps w (|u_lo| + |u_hi| + 2 |g|) (|lam_lo| + |lam_hi|)  per face, 4 eps a |u lam| per cell, on what an
    evaluation of the same formulas in another order may differ by.  On a wall face there is one cell; w is b/h^2 between cells and on a
    Dirichlet wall, (b/h) (2/(2 + t)) on a Neumann / Robin wall, where |u_c| counts kappa times.  faces: the six kinds (None: all Dirichlet);
    kappa: the (6,N,N) array of the Robin faces."""
    w2, w, wn = b * (1.0 / (h * h)), (2.0 * b) * (1.0 / (h * h)), b * (1.0 / h)
    out = [(a * (u * lam), 4.0 * EPS * a * np.abs(u * lam)) if a != 0.0 else (None, None)]
    zero = np.zeros((n, n))
    for axis in range(3):
        U, L = _along(u, axis), _along(lam, axis)
        if bc == "periodic":
            ulo, llo = np.roll(U, 1, axis=0), np.roll(L, 1, axis=0)
            G = w2 * ((ulo - U) * (llo - L))
            bound = 16.0 * EPS * w2 * (np.abs(ulo) + np.abs(U)) * (np.abs(llo) + np.abs(L))
        else:
            G, bound = np.empty((n + 1,) + U.shape[1:]), np.empty((n + 1,) + U.shape[1:])
            G[1:n] = w2 * ((U[:-1] - U[1:]) * (L[:-1] - L[1:]))
            bound[1:n] = 16.0 * EPS * w2 * (np.abs(U[:-1]) + np.abs(U[1:])) * (np.abs(L[:-1]) + np.abs(L[1:]))
            for side, cell, entry in ((0, 0, 0), (1, n - 1, n)):
                face = 2 * axis + side
                gv = zero if g is None else g[face]
                kind = D if faces is None else faces[face]
                if kind == D:
                    G[entry] = (w * (U[cell] - gv)) * L[cell]
                    bound[entry] = 16.0 * EPS * w2 * (np.abs(U[cell]) + 2.0 * np.abs(gv)) * np.abs(L[cell])
                else:
                    kap = kappa[face] if (kind == R and kappa is not None) else zero
                    t = kap * h
                    G[entry] = ((wn * (2.0 / (2.0 + t))) * (kap * U[cell] - gv)) * L[cell]
                    bound[entry] = 16.0 * EPS * (wn * (2.0 / (2.0 + t))) * (kap * np.abs(U[cell]) + 2.0 * np.abs(gv)) * np.abs(L[cell])
        out.append((np.ascontiguousarray(np.moveaxis(G, 0, 2 - axis)), np.ascontiguousarray(np.moveaxis(bound, 0, 2 - axis))))
    return out


def dot(G, d):
    """(sum_p G_p d_p, sum_p |G_p d_p|) over the arrays that are not None, exactly summed."""
    terms = np.concatenate([(x * y).ravel() for x, y in zip(G, d) if x is not None])
    return math.fsum(terms), math.fsum(np.abs(terms))


def random_direction(coef, seed, positive=False):
    """One array per coefficient array (None where that is None) with entries in (-1/2, 1/2), or in (0, 1/2) when positive."""
    rng = np.random.default_rng(seed)
    out = []
    for c in coef:
        if c is None:
            out.append(None)
            continue
        r = rng.random(c.shape)
        out.append(0.5 * r if positive else r - 0.5)
    return out


def shifted(coef, d, eps):
    return [None if c is None else c + eps * x for c, x in zip(coef, d)]
