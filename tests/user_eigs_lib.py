"""Helpers of the eigenmode tests (Solver.eigs): the problems as data, the dense operator of a small solver column by column
through Solver.apply, the exact pencil spectrum from numpy.linalg.eigh, and the two measures of a returned pair the tests recompute themselves.

With rho = |A x - mu M x|_{M^-1} / |x|_M some exact eigenvalue of the pencil (A, M) lies within rho of mu (the residual bound of a symmetric
pencil in the M inner product: M^-1/2 A M^-1/2 is symmetric, y = M^1/2 x, and |B y - mu y| / |y| bounds the distance of mu to B's spectrum).
"""
import numpy as np

from user_cells_lib import block_field
from user_flux_lib import SOLVERS, kappa_for
from user_problem_lib import random_coefficients

EPS = np.finfo(np.float64).eps
B = 0.7
# name -> (bc key of user_flux_lib.SOLVERS, a, what the coefficients are)
CASES = {"dirichlet": ("dirichlet", 1.3, "smooth"), "corners": ("corners", 1.3, "smooth"), "robin": ("robin", 0.9, "smooth"),
         "neumann": ("neumann", 0.9, "smooth"), "periodic": ("periodic", 1.3, "smooth"), "poisson": ("dirichlet", 0.0, "smooth"),
         "random-alpha": ("dirichlet", 2.0, "alpha"), "contrast": ("dirichlet", 0.5, "contrast")}


def set_case(s, name, n, seed=7):
    """The coefficients of CASES[name] into the solver; returns alpha (None on a Poisson solver)."""
    solver, a, kind = CASES[name]
    bc = "periodic" if solver == "periodic" else "dirichlet"
    alpha, bi, bj, bk = random_coefficients(n, bc, a != 0.0, seed)
    kappa = kappa_for(solver, n)
    if kind == "alpha":
        alpha = 0.5 + np.random.default_rng(seed + 1).random((n, n, n))
    if kind == "contrast":
        alpha = 0.5 + np.random.default_rng(seed + 1).random((n, n, n))
        s.set_cell_coefficients(alpha, block_field(n, seed + 2, jump=100.0), mean="harmonic", robin=kappa)
    else:
        s.set_coefficients(alpha, bi, bj, bk, robin=kappa)
    return alpha


def bc_of(name):
    return SOLVERS[CASES[name][0]]


def dense_operator(s):
    """A as a dense (n^3, n^3) array, column by column: A e_c = s.apply(e_c)."""
    n = s.n
    cells = n ** 3
    A = np.empty((cells, cells))
    e, y = np.zeros((n, n, n)), np.empty((n, n, n))
    flat = e.reshape(-1)
    for c in range(cells):
        flat[c] = 1.0
        s.apply(e, out=y)
        A[:, c] = y.reshape(-1)
        flat[c] = 0.0
    return A


def exact_spectrum(A, m):
    """The eigenvalues of the pencil (A, diag(m)), ascending: eigh of M^-1/2 A M^-1/2 (symmetrised: A's columns come from a symmetric operator)."""
    d = 1.0 / np.sqrt(m)
    Bm = d[:, None] * A * d[None, :]
    return np.linalg.eigvalsh(0.5 * (Bm + Bm.T))


def rho(Ax, m, mu, x):
    r = Ax - mu * m * x
    return float(np.sqrt(np.sum(r * r / m)) / np.sqrt(np.sum(m * x * x)))


def residual_measure(Ax, m, mu, x):
    """EigInfo.residuals' definition, and the rounding of either side's evaluation of it: at most ~10 terms per cell each, every one within eps of
    |A| |x| + mu |M x| there, so 32 eps of the largest such sum over the same denominator."""
    r = Ax - mu * m * x
    den = mu * np.abs(m * x).max()
    return float(np.abs(r).max() / den)


def closed_form(n, b, h, k, kind):
    """The k lowest lambda of the constant-coefficient K: (4 b / h^2) sum_d sin^2(p_d pi / 2N) with p_d >= 1 (Dirichlet) or >= 0 (Neumann), and
    (4 b / h^2) sum_d sin^2(p_d pi / N) over all integer p_d (periodic)."""
    if kind == "periodic":
        one = [np.sin(p * np.pi / n) ** 2 for p in range(-3, 4)]
    else:
        one = [np.sin(p * np.pi / (2 * n)) ** 2 for p in range(1 if kind == "dirichlet" else 0, 6)]
    return np.array(sorted((4.0 * b / h ** 2) * (x + y + z) for x in one for y in one for z in one)[:k])
