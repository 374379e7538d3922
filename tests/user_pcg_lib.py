"""Helpers of the method="pcg" tests (hpgmg_amd/problem.py): the contrast problem.

beta is 1 in the cells of the N^3 grid except in random blocks of 4^3 cells (30 % of the blocks, chosen with `seed`), where it is `contrast`; the
block pattern is shifted by (1, 2, 3) cells along (i, j, k), periodically, so that the jumps do not lie on the faces of any coarse cell.  The face
between two cells takes the harmonic mean of their values; a domain face takes its cell's value.  Poisson (a = 0, b = 1), Dirichlet walls, a right-hand
side uniform in [-1, 1].
"""
import numpy as np


def contrast_cells(n, contrast, seed=3, block=4, fill=0.3, shift=(1, 2, 3)):
    """The cell values of beta, indexed [k][j][i]."""
    rng = np.random.default_rng(seed)
    nb = (n + block - 1) // block
    chosen = rng.random((nb, nb, nb)) < fill
    cells = np.where(np.kron(chosen, np.ones((block,) * 3, dtype=bool))[:n, :n, :n], float(contrast), 1.0)
    return np.ascontiguousarray(np.roll(cells, shift=(shift[2], shift[1], shift[0]), axis=(0, 1, 2)))


def contrast_problem(n, contrast, seed=3):
    """(beta_i, beta_j, beta_k, f) of the Dirichlet problem: the face arrays are one longer along their axis (hpgmg_amd/problem.py)."""
    cells = contrast_cells(n, contrast, seed)
    betas = []
    for ax in (2, 1, 0):                                      # numpy axis of i, j, k
        lo = np.take(cells, np.arange(n - 1), axis=ax)
        hi = np.take(cells, np.arange(1, n), axis=ax)
        inner = 2.0 * lo * hi / (lo + hi)
        first = np.take(cells, [0], axis=ax)
        last = np.take(cells, [n - 1], axis=ax)
        betas.append(np.ascontiguousarray(np.concatenate([first, inner, last], axis=ax)))
    f = np.random.default_rng(seed + 1000).random((n, n, n)) * 2.0 - 1.0
    return betas[0], betas[1], betas[2], f
