"""Helpers of the cell-centred conductivity tests (Solver.set_cell_coefficients, Solver.cell_sensitivity, hpgmg_amd.autograd.solve_cells;
DESIGN.md §11.10): NumPy restatements, in the written order of include/hpgmg_boundary_math.h (bnd_mean, bnd_mean_dlo, bnd_mean_dhi), of the face
mean of a cell field and of its transpose, the gather of face sensitivities back to cells.  NumPy evaluates one IEEE operation per call and every
build of the library has -ffp-contract=off, so both have the library's bits.  They share no code with it: slices of dense arrays, not boxes.

lo is the cell with the smaller index along the axis, hi the other one; on a periodic wrap face lo = cell N-1 and hi = cell 0.  A domain wall face
of any kind takes its cell's own value, derivative 1.0.
"""
import numpy as np

import hpgmg_amd as H
from user_flux_lib import _along

MEANS = ["harmonic", "arithmetic"]
# a bad k: what set_cell_coefficients and cell_sensitivity report for it.  In a 24^3 grid in boxes of 8 cell (9, 12, 10) lies in the middle box.
STATUS_CASES = [                                                        # (name, [(cell (k, j, i), value)], mean, status, what the message says)
    ("nan in the first cell", [((0, 0, 0), np.nan)], "harmonic", H.USER_NOT_FINITE, "not finite"),
    ("nan in the last cell", [((-1, -1, -1), np.nan)], "arithmetic", H.USER_NOT_FINITE, "not finite"),
    ("nan in a middle box", [((9, 12, 10), np.nan)], "harmonic", H.USER_NOT_FINITE, "not finite"),
    ("zero next to a positive cell", [((9, 12, 10), 0.0)], "harmonic", H.USER_OUT_OF_RANGE, "out of range"),
    ("negative next to a positive cell", [((9, 12, 10), -1.0)], "harmonic", H.USER_OUT_OF_RANGE, "out of range"),
    ("negative, arithmetic", [((0, 7, 8), -1.0)], "arithmetic", H.USER_OUT_OF_RANGE, "out of range"),
    ("lo * hi overflows", [((9, 12, 10), 1e200), ((9, 12, 11), 1e200)], "harmonic", H.USER_NOT_FINITE, "harmonic mean.*overflows"),
    ("the mean underflows", [((9, 12, 10), 1e-200), ((9, 13, 10), 1e-200)], "harmonic", H.USER_OUT_OF_RANGE, "harmonic mean.*underflows"),
]


def planted(n, plants):
    k = np.ones((n, n, n))
    for at, value in plants:
        k[at] = value
    return k


def mean_of(mean, lo, hi):
    return (2.0 * (lo * hi)) / (lo + hi) if mean == "harmonic" else 0.5 * (lo + hi)


def mean_dlo(mean, lo, hi):
    """d mean / d lo."""
    if mean != "harmonic":
        return np.full(np.shape(lo), 0.5)
    t = hi / (lo + hi)
    return 2.0 * (t * t)


def mean_dhi(mean, lo, hi):
    return mean_dlo(mean, hi, lo)


def block_field(n, seed, jump=100.0):
    """k = 0.5 + random, times a 100 : 1 block jump in one octant."""
    k = 0.5 + np.random.default_rng(seed).random((n, n, n))
    k[n // 2:, n // 2:, n // 2:] *= jump
    return k


def face_mean(n, bc, k, mean):
    """The three face arrays (beta_i, beta_j, beta_k) of the cell field k, in set_coefficients' shapes."""
    out = []
    for axis in range(3):
        K = _along(k, axis)
        if bc == "periodic":
            F = mean_of(mean, np.roll(K, 1, axis=0), K)
        else:
            F = np.empty((n + 1,) + K.shape[1:])
            F[0], F[n] = K[0], K[n - 1]
            F[1:n] = mean_of(mean, K[:-1], K[1:])
        out.append(np.ascontiguousarray(np.moveaxis(F, 0, 2 - axis)))
    return out


def cell_terms(n, bc, k, mean, G_i, G_j, G_k):
    """The six products G D of every cell, in the order i-low, i-high, j-low, j-high, k-low, k-high, and the six D."""
    terms, factors = [], []
    for axis, G in enumerate((G_i, G_j, G_k)):
        K, Gf = _along(k, axis), _along(G, axis)
        if bc == "periodic":
            below, above = np.roll(K, 1, axis=0), np.roll(K, -1, axis=0)
            D_lo, D_hi = mean_dhi(mean, below, K), mean_dlo(mean, K, above)
            G_lo, G_hi = Gf, np.roll(Gf, -1, axis=0)
        else:
            D_lo, D_hi = np.ones(K.shape), np.ones(K.shape)
            D_lo[1:] = mean_dhi(mean, K[:-1], K[1:])
            D_hi[:-1] = mean_dlo(mean, K[:-1], K[1:])
            G_lo, G_hi = Gf[:-1], Gf[1:]
        for Gs, D in ((G_lo, D_lo), (G_hi, D_hi)):
            terms.append(np.moveaxis(Gs * D, 0, 2 - axis))      # a wall: G * 1.0, which has G's bits
            factors.append(np.moveaxis(D, 0, 2 - axis))
    return terms, factors


def cell_gather(n, bc, k, mean, G_i, G_j, G_k):
    """d_k: per cell ((((G_il D_il + G_ih D_ih) + G_jl D_jl) + G_jh D_jh) + G_kl D_kl) + G_kh D_kh, left to right."""
    t, _ = cell_terms(n, bc, k, mean, G_i, G_j, G_k)
    return np.ascontiguousarray(((((t[0] + t[1]) + t[2]) + t[3]) + t[4]) + t[5])
