"""Helpers of the boundary-value tests (Solver(..., boundary=)): T(g) as a NumPy array, and a manufactured problem with a smooth solution
that is non-zero on every face and a smooth variable beta.

T restates include/hpgmg_operators.h / DESIGN.md §11: a boundary cell's ghost is 2 g - u, so each domain face f of a cell moves
2 b h^-2 beta_f g_f to the right-hand side (A0 u = f + T(g), A0 the homogeneous operator of user_problem_lib.assemble).
"""
import numpy as np


def lift(n, b, h, beta_i, beta_j, beta_k, g):
    """T(g) on the (N,N,N) [k][j][i] grid (summed in NumPy's order: compare to 1e-13, not bitwise)."""
    c = 2.0 * b / (h * h)
    T = np.zeros((n, n, n))
    T[:, :, 0] += c * beta_i[:, :, 0] * g[0]
    T[:, :, -1] += c * beta_i[:, :, n] * g[1]
    T[:, 0, :] += c * beta_j[:, 0, :] * g[2]
    T[:, -1, :] += c * beta_j[:, n, :] * g[3]
    T[0, :, :] += c * beta_k[0, :, :] * g[4]
    T[-1, :, :] += c * beta_k[n, :, :] * g[5]
    return T


# u* = sin(1.3x + 0.4) cos(0.7y - 0.2) exp(0.5z) + 0.3, beta = 1 + 0.5 sin(2x + 1) cos(y) cos(z/2)^2, alpha = 1 + x^2/2 + yz/4
def exact(x, y, z):
    return np.sin(1.3 * x + 0.4) * np.cos(0.7 * y - 0.2) * np.exp(0.5 * z) + 0.3


def _beta(x, y, z):
    return 1.0 + 0.5 * np.sin(2 * x + 1) * np.cos(y) * np.cos(0.5 * z) ** 2


def _alpha(x, y, z):
    return 1.0 + 0.5 * x * x + 0.25 * y * z


def manufactured(n, a, b):
    """(alpha or None, beta_i, beta_j, beta_k, f, u* at the cell centres) on the unit cube, h = 1/n; beta sampled at face centres."""
    h = 1.0 / n
    c = (np.arange(n) + 0.5) * h
    fc = np.arange(n + 1) * h
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")

    def on(zs, ys, xs):
        zz, yy, xx = np.meshgrid(zs, ys, xs, indexing="ij")
        return np.ascontiguousarray(_beta(xx, yy, zz))

    bi, bj, bk = on(c, c, fc), on(c, fc, c), on(fc, c, c)
    s, co = np.sin(1.3 * X + 0.4), np.cos(1.3 * X + 0.4)
    cy, sy, e = np.cos(0.7 * Y - 0.2), np.sin(0.7 * Y - 0.2), np.exp(0.5 * Z)
    ux, uy, uz = 1.3 * co * cy * e, -0.7 * s * sy * e, 0.5 * s * cy * e
    lap = (-1.69 - 0.49 + 0.25) * s * cy * e
    cz = np.cos(0.5 * Z)
    bx = np.cos(2 * X + 1) * np.cos(Y) * cz ** 2
    by = -0.5 * np.sin(2 * X + 1) * np.sin(Y) * cz ** 2
    bz = -0.5 * np.sin(2 * X + 1) * np.cos(Y) * cz * np.sin(0.5 * Z)
    u = exact(X, Y, Z)
    f = -b * (_beta(X, Y, Z) * lap + bx * ux + by * uy + bz * uz)
    alpha = None
    if a != 0.0:
        alpha = np.ascontiguousarray(_alpha(X, Y, Z))
        f = f + a * alpha * u
    return alpha, bi, bj, bk, np.ascontiguousarray(f), u
