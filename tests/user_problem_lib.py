"""Helpers of the user-problem tests (hpgmg_amd/problem.py): the operator as a SciPy matrix, random coefficients, and the benchmark's
problem as dense arrays.

The matrix restates operators.7pt.c's variable-coefficient apply_op_ijk with boundary_fd.c's p1 Dirichlet rule as the plugin applies it:
    (A u)_c = a alpha_c u_c + b h^-2 sum over the six faces f of c: beta_f (u_c - u_nb(f)),
where the neighbour across a Dirichlet domain face is the ghost value -u_c, and across a periodic one the cell on the other side.
"""
import ctypes

import numpy as np
import scipy.sparse as sp

import hpgmg_amd as H


def face_shape(n, bc, axis):
    shape = [n, n, n]
    if bc == "dirichlet":
        shape[2 - axis] += 1
    return tuple(shape)


def assemble(n, bc, a, b, h, alpha, beta_i, beta_j, beta_k):
    """SciPy CSR matrix of the operator on the [k][j][i]-ordered cells."""
    c = b / (h * h)
    idx = np.arange(n ** 3).reshape(n, n, n)
    diag = np.zeros((n, n, n))
    if alpha is not None:
        diag += a * alpha
    rows, cols, vals = [], [], []
    for axis, beta in ((0, beta_i), (1, beta_j), (2, beta_k)):
        ax = 2 - axis                                          # numpy axis of i / j / k
        for side in (-1, +1):
            # the face between the cell and its neighbour on `side`: low face = beta[cell], high face = beta[cell + 1] (periodic: wraps)
            if side < 0:
                face = beta.take(np.arange(n), axis=ax)
            else:
                face = beta.take((np.arange(n) + 1) % (n if bc == "periodic" else n + 1), axis=ax)
            pos = np.arange(n) + side
            inside = (pos >= 0) & (pos < n)
            shape = [1, 1, 1]
            shape[ax] = n
            inside3 = np.broadcast_to(inside.reshape(shape), (n, n, n))
            if bc == "periodic":
                nb = idx.take(pos % n, axis=ax)
                diag += c * face
                rows.append(idx.ravel()); cols.append(nb.ravel()); vals.append((-c * face).ravel())
            else:
                nb = idx.take(np.clip(pos, 0, n - 1), axis=ax)
                diag += np.where(inside3, c * face, 2.0 * c * face)
                m = inside3.ravel()
                rows.append(idx.ravel()[m]); cols.append(nb.ravel()[m]); vals.append((-c * face).ravel()[m])
    rows.append(idx.ravel()); cols.append(idx.ravel()); vals.append(diag.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3))
    return A.tocsr()


def smooth_field(shape, rng, low, high):
    """A smooth positive random field: a few low Fourier modes scaled into [low, high]."""
    grids = np.meshgrid(*[np.linspace(0.0, 1.0, s) for s in shape], indexing="ij")
    v = np.zeros(shape)
    for _ in range(4):
        kx, ky, kz = rng.integers(1, 4, size=3)
        ph = rng.random(3) * 2 * np.pi
        v += rng.random() * np.sin(kx * np.pi * grids[0] + ph[0]) * np.sin(ky * np.pi * grids[1] + ph[1]) * np.sin(kz * np.pi * grids[2] + ph[2])
    v = (v - v.min()) / (v.max() - v.min() + 1e-300)
    return np.ascontiguousarray(low + (high - low) * v)


def random_coefficients(n, bc, helmholtz, seed):
    rng = np.random.default_rng(seed)
    alpha = smooth_field((n, n, n), rng, 0.5, 2.0) if helmholtz else None
    betas = [smooth_field(face_shape(n, bc, axis), rng, 0.5, 3.0) for axis in range(3)]
    return alpha, betas[0], betas[1], betas[2]


def benchmark_arrays(lib, boxes_in_i, box_dim, bc, a, b):
    """The benchmark's problem (initialize_problem, before any mean shift) as dense arrays: interior cells, plus face N of each beta taken
    from the ghost layer of the boxes on the high domain face (Dirichlet)."""
    n = boxes_in_i * box_dim
    h = 1.0 / n
    ghosts, nv = lib.stencil_get_radius(), lib.hpgmg_vectors_reserved()
    L = lib.hpgmg_level_create(boxes_in_i, box_dim, ghosts, nv, H.BC_PERIODIC if bc == "periodic" else H.BC_DIRICHLET, 0, 1, h)
    try:
        lib.initialize_problem(L, h, a, b)
        info = (ctypes.c_int * H.INFO_COUNT)()
        lib.hpgmg_level_info(L, info)
        jS, kS, vol, nb = info[H.INFO_JSTRIDE], info[H.INFO_KSTRIDE], info[H.INFO_VOLUME], info[H.INFO_NUM_MY_BOXES]
        w, g, d = box_dim + 2 * ghosts, ghosts, box_dim
        out = {"f": np.zeros((n, n, n)), "alpha": np.zeros((n, n, n)) if a != 0.0 else None}
        for axis, name in enumerate(("beta_i", "beta_j", "beta_k")):
            out[name] = np.zeros(face_shape(n, bc, axis))
        ids = {"f": H.VECTOR_F, "alpha": H.VECTOR_ALPHA, "beta_i": H.VECTOR_BETA_I, "beta_j": H.VECTOR_BETA_J, "beta_k": H.VECTOR_BETA_K}
        buf = np.empty(vol)
        for box in range(nb):
            low = (ctypes.c_int * 3)()
            lib.hpgmg_level_box_low(L, box, low)
            li, lj, lk = low
            for name, vid in ids.items():
                if out[name] is None:
                    continue
                lib.hpgmg_level_read_vector(L, box, vid, buf.ctypes.data)
                pad = buf[: w * kS].reshape(w, kS)[:, : w * jS].reshape(w, w, jS)
                e = [d, d, d]                                  # extent along k, j, i
                if name.startswith("beta") and bc == "dirichlet":
                    ax = {"beta_i": 2, "beta_j": 1, "beta_k": 0}[name]
                    if (li, lj, lk)[2 - ax] + d == n:
                        e[ax] += 1
                out[name][lk:lk + e[0], lj:lj + e[1], li:li + e[2]] = pad[g:g + e[0], g:g + e[1], g:g + e[2]]
        return out
    finally:
        lib.hpgmg_level_destroy(L)
