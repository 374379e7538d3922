"""Helpers of the Robin-wall tests (Solver(n, bc=<6-tuple with "convective">), set_coefficients(..., robin=kappa)): the wall mixes, a smooth positive
kappa sampled per face, the operator A_R and the lift T(g) as SciPy / NumPy restatements, and the per-level wall arrays.

Restates DESIGN.md §11.5.  On a Robin wall  du/dn + kappa u = g  is discretised with du/dn = (u_g - u) / h and u_wall = (u_g + u) / 2, so with
t = kappa h the ghost is u_g = c u + d g, c = (2 - t) / (2 + t), d = 2 h / (2 + t).  The wall term (b/h^2) beta_wall (u - u_g) then adds
(b/h^2) beta_wall 2 t / (2 + t) to the diagonal -- the Dirichlet assembly with a wall beta of beta_wall t / (2 + t) -- and
(b/h) beta_wall g 2 / (2 + t) to the right-hand side.
"""
import ctypes

import numpy as np

import hpgmg_amd as H
from user_neumann_lib import wall_slices
from user_problem_lib import assemble

D, N, R = "dirichlet", "neumann", "convective"      # a Robin wall is spelled "convective" in bc=
ONE = (D, D, D, R, D, D)                 # one Robin face (j-high)
SIDES = (D, D, R, R, N, N)               # Dirichlet i-walls, Robin j-walls, Neumann k-walls
ALL = (R,) * 6
CORNERS = (R, D, N, R, R, D)             # edges R-N (i-low, j-low), R-R (i-low, j-high), R-D (i-low, k-high); corner D-N-R (i-high, j-low, k-low)
WALLS = {"one": ONE, "sides": SIDES, "all": ALL, "corners": CORNERS}


def neumann_of(faces):
    """The same walls with every Robin face Neumann: what kappa = 0 must reproduce bit for bit."""
    return tuple(N if kind == R else kind for kind in faces)


def mask_of(faces):
    return sum(1 << f for f, kind in enumerate(faces) if kind != D)


def kappa_field(x, y, z):
    return 1.0 + x + 0.5 * np.sin(2.0 * y) * np.cos(z)


def sample_faces(n, h, fn):
    """fn(x, y, z) at the 6 n^2 face centres, in the layout of `boundary`."""
    c = (np.arange(n) + 0.5) * h
    slow, fast = np.meshgrid(c, c, indexing="ij")
    out = np.empty((6, n, n))
    for face in range(6):
        wall = np.full((n, n), n * h if face & 1 else 0.0)
        x, y, z = (wall, fast, slow) if face < 2 else (fast, wall, slow) if face < 4 else (fast, slow, wall)
        out[face] = fn(x, y, z)
    return out


def kappa_of(n, faces, h=None):
    """The smooth kappa on the Robin faces, 0 on the others (as the solver stores it)."""
    k = sample_faces(n, h or 1.0 / n, kappa_field)
    for f, kind in enumerate(faces):
        if kind != R:
            k[f] = 0.0
    return k


def assemble_robin(n, faces, kappa, a, b, h, alpha, beta_i, beta_j, beta_k):
    """A_R as a SciPy matrix: the Dirichlet assembly with beta t / (2 + t) on a Robin wall, 0 on a Neumann wall."""
    betas = [beta_i.copy(), beta_j.copy(), beta_k.copy()]
    for f, (which, idx) in enumerate(wall_slices(n)):
        if faces[f] == N:
            betas[which][idx] = 0.0
        elif faces[f] == R:
            t = kappa[f] * h
            betas[which][idx] = betas[which][idx] * (t / (2.0 + t))
    return assemble(n, "dirichlet", a, b, h, alpha, *betas)


def lift_robin(n, faces, kappa, b, h, beta_i, beta_j, beta_k, g):
    """T(g): 2 b h^-2 beta g on a Dirichlet face, b h^-1 beta gn on a Neumann face, b h^-1 beta g 2 / (2 + kappa h) on a Robin face."""
    betas = (beta_i, beta_j, beta_k)
    s = slice(None)
    cells = [(s, s, 0), (s, s, -1), (s, 0, s), (s, -1, s), (0, s, s), (-1, s, s)]
    T = np.zeros((n, n, n))
    for f, (which, idx) in enumerate(wall_slices(n)):
        if faces[f] == D:
            T[cells[f]] += 2.0 * b / (h * h) * betas[which][idx] * g[f]
        elif faces[f] == N:
            T[cells[f]] += b / h * betas[which][idx] * g[f]
        else:
            T[cells[f]] += b / h * betas[which][idx] * g[f] * (2.0 / (2.0 + kappa[f] * h))
    return T


def wall_array(n, beta_i, beta_j, beta_k):
    """The fine level's wall-beta array: each face's beta in the layout of `boundary`."""
    betas = (beta_i, beta_j, beta_k)
    return np.stack([betas[which][idx] for which, idx in wall_slices(n)])


def restrict_faces(a):
    """hpgmg_boundary_restrict, in its written order: ((e[2q][2p] + e[2q][2p+1]) + e[2q+1][2p]) + e[2q+1][2p+1]) * 0.25"""
    return (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * 0.25


def level_vector(lib, L, vid):
    """(level info, [(box low, the padded box of vector vid)])"""
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


def beta_cells(info, axis):
    """Offsets into a padded box of the beta entries the operator reads: 0 .. dim along the array's axis (dim: the high face), 0 .. dim-1
    across, as [along][across0][across1] with across0 < across1 the other two axes."""
    dim, gh, strides = info[H.INFO_BOX_DIM], info[H.INFO_GHOSTS], (1, info[H.INFO_JSTRIDE], info[H.INFO_KSTRIDE])
    across = [x for x in range(3) if x != axis]
    idx = np.arange(dim + 1)[:, None, None] * strides[axis]
    idx = idx + np.arange(dim)[None, :, None] * strides[across[0]] + np.arange(dim)[None, None, :] * strides[across[1]]
    return idx + gh * sum(strides)


def wall_entries(face_array, face, low, dim):
    """The (dim, dim) block of a level's boundary array under a box at `low`, as [across0][across1] of beta_cells (the array is [q][p] with
    p the faster axis, i.e. [across1][across0])."""
    axis = face // 2
    across = [x for x in range(3) if x != axis]
    block = face_array[face][low[across[1]]:low[across[1]] + dim, low[across[0]]:low[across[0]] + dim]
    return block.T


def levels_of(lib, s):
    G = lib.hpgmg_solver_mg(lib.hpgmg_user_solver_of(s._ptr))
    return [lib.hpgmg_mg_level(G, l) for l in range(lib.hpgmg_mg_num_levels(G))]


def level_walls(lib, s):
    """Per level: its three beta vectors on every box (level_vector) and its eigenvalue estimate, for bitwise comparisons."""
    out = []
    for L in levels_of(lib, s):
        vecs = [level_vector(lib, L, vid)[1] for vid in (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)]
        out.append((vecs, lib.hpgmg_level_eigenvalue(L)))
    return out
