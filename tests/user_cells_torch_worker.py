"""Child process of tests/test_gpu_user_cells.py: torch first, then the project's libraries (one HIP runtime).  Solver.set_cell_coefficients and
Solver.cell_sensitivity on torch tensors must equal the NumPy path bitwise and write out= in place; hpgmg_amd.autograd.solve_cells must give, bitwise,
the gradients of the manual composition (lam for f, -d_alpha and -d_k of cell_sensitivity(u, lam, k, boundary=g)) on a second solver and on the CPU
oracle; its three errors raise; and its k.grad agrees with the existing route -- the face mean written in torch and fed to autograd.solve -- per cell
within 32 eps sum_f |G_f| |D_f|: two orders of a six-term sum (at most 10 eps) and two roundings of D from a different expression."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd import autograd  # noqa: E402
from hpgmg_amd.problem import Solver, hip_runtimes_mapped  # noqa: E402
from hpgmg_testlib import Backend  # noqa: E402
from user_cells_lib import MEANS, block_field, cell_terms  # noqa: E402
from user_flux_lib import EPS, SOLVERS, boundary_for, kappa_for  # noqa: E402

B = 0.7


def refused(call, *args, kind=ValueError, **kwargs):
    try:
        call(*args, **kwargs)
    except kind as e:
        return str(e)
    raise AssertionError("the call was accepted")


def same(t, a):
    """A tensor and a NumPy array hold the same bits (or both are None)."""
    if t is None or a is None:
        return t is None and a is None
    return t.cpu().numpy().tobytes() == a.tobytes()


def _fields(n, a, seed):
    rng = np.random.default_rng(seed)
    alpha = rng.random((n, n, n)) + 0.5 if a != 0.0 else None
    return alpha, block_field(n, seed + 1), rng.random((n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5


def tensors_equal_numpy(dev, T):
    n = 64
    for (name, a), mean in zip((("corners", 1.3), ("periodic", 0.0)), MEANS):
        alpha, k, u, lam = _fields(n, a, 181)
        kappa, g = kappa_for(name, n), boundary_for(name, n, 182)
        with Solver(n, box_dim=32, bc=SOLVERS[name], a=a, b=B) as s, Solver(n, box_dim=32, bc=SOLVERS[name], a=a, b=B) as t:
            s.set_cell_coefficients(alpha, k, mean=mean, robin=kappa)
            t.set_cell_coefficients(T(alpha), T(k), mean=mean, robin=T(kappa))
            assert same(t.apply(T(u), boundary=T(g)), s.apply(u, boundary=g))
            host = s.cell_sensitivity(u, lam, k, mean=mean, boundary=g)
            got = t.cell_sensitivity(T(u), T(lam), T(k), mean=mean, boundary=T(g))
            assert (got[0] is None) == (a == 0.0)
            for q_h, q_d in zip(host, got):
                assert q_d is None or (isinstance(q_d, torch.Tensor) and q_d.device == dev and q_d.dtype == torch.float64)
                assert same(q_d, q_h)
            into = tuple(None if q is None else torch.full_like(q, float("nan")) for q in got)
            back = t.cell_sensitivity(T(u), T(lam), T(k), mean=mean, boundary=T(g), out=into)
            assert all(x is y for x, y in zip(back, into))
            for q_h, q_d in zip(host, into):
                assert same(q_d, q_h)
            if alpha is not None:
                assert refused(t.set_cell_coefficients, T(alpha), k, mean=mean, robin=T(kappa)).startswith("alpha: a torch array among numpy arrays")
            assert refused(t.cell_sensitivity, T(u), T(lam), k).startswith("k: a numpy array among torch arrays")
            assert refused(t.cell_sensitivity, u, lam, T(k)).startswith("k: a torch array among numpy arrays")
            assert refused(t.cell_sensitivity, T(u), T(lam), T(k), out=host).startswith(("out[0]: a numpy", "out[1]: a numpy"))
            assert refused(t.cell_sensitivity, T(u), T(lam), T(k), out=(got[0], got[1].float())).startswith("out[1]: dtype")
            bad = k.copy()
            bad[5, 6, 7] = -1.0
            assert refused(t.set_cell_coefficients, T(alpha), T(bad), mean=mean, robin=T(kappa)).startswith("k: is out of range")
            t.set_cell_coefficients(T(alpha), T(k), mean=mean, robin=T(kappa))
            assert refused(t.cell_sensitivity, T(u), T(lam), T(bad), mean=mean).startswith("k: is out of range")


def torch_face_mean(k, mean):
    """The three face arrays of a Dirichlet-shaped solver from the cell tensor k, differentiable: the route a user of autograd.solve had to write."""
    out = []
    for dim in (2, 1, 0):                                       # beta_i varies along the last index
        n = k.shape[dim]
        lo, hi = k.narrow(dim, 0, n - 1), k.narrow(dim, 1, n - 1)
        inner = (2.0 * (lo * hi)) / (lo + hi) if mean == "harmonic" else 0.5 * (lo + hi)
        out.append(torch.cat([k.narrow(dim, 0, 1), inner, k.narrow(dim, n - 1, 1)], dim=dim).contiguous())
    return out


def autograd_equals_the_manual_composition(dev, T, oracle):
    n, box_dim, rtol = 32, 16, 1e-10
    for (name, a), mean in zip((("dirichlet", 1.3), ("corners", 0.0)), MEANS):
        alpha, k, f, w = _fields(n, a, 191)
        kappa, g = kappa_for(name, n), boundary_for(name, n, 192)
        leaves = [None if alpha is None else T(alpha).requires_grad_(True), T(k).requires_grad_(True)]
        tf = T(f).requires_grad_(True)
        with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B) as s:
            u = autograd.solve_cells(s, tf, *leaves, mean=mean, boundary=T(g), robin=T(kappa), method="mg", rtol=rtol)
            assert isinstance(u, torch.Tensor) and u.requires_grad
            (T(w) * u).sum().backward()                  # grad_u is exactly w
            assert same(s.get_solution(torch.empty_like(u)), tf.grad.cpu().numpy())      # backward leaves lam as the last solution
        grads = [tf.grad] + [None if x is None else x.grad for x in leaves]
        # the manual composition on a second solver of the product, from tensors, and on the oracle, from NumPy arrays
        for lib, put in ((None, T), (oracle, lambda v: v)):
            with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B, lib=lib) as m:
                m.set_cell_coefficients(put(alpha), put(k), mean=mean, robin=put(kappa))
                u2, info = m.solve(put(f), method="mg", rtol=rtol, boundary=put(g))
                assert info.converged
                lam, info = m.solve(put(w), method="mg", rtol=rtol)
                assert info.converged
                G = m.cell_sensitivity(u2, lam, put(k), mean=mean, boundary=put(g))
                faces = m.sensitivity(u2, lam, boundary=put(g))
            numpy_of = (lambda v: v.cpu().numpy()) if lib is None else (lambda v: v)
            assert same(u.detach(), numpy_of(u2)), (name, "u")
            assert same(grads[0], numpy_of(lam)), (name, "f")
            for slot, (got, ref) in enumerate(zip(grads[1:], G)):
                assert same(got, None if ref is None else -numpy_of(ref)), (name, slot)
        # the existing route: the face mean in torch, autograd.solve, and torch's own chain rule through the mean
        tk = T(k).requires_grad_(True)
        with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B) as s:
            v = autograd.solve(s, T(f), T(alpha), *torch_face_mean(tk, mean), boundary=T(g), robin=T(kappa), method="mg", rtol=rtol)
            assert same(v.detach(), u.detach().cpu().numpy()), (name, "the torch face mean gives other coefficients")
            (T(w) * v).sum().backward()
        terms, _ = cell_terms(n, "dirichlet", k, mean, *[np.abs(q) for q in faces[1:]])       # |G_f| |D_f| per cell and face (faces: the oracle's, NumPy)
        bound = 32.0 * EPS * (((((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]) + terms[5])
        miss = np.abs(tk.grad.cpu().numpy() - leaves[1].grad.cpu().numpy())
        print(f"{name} {mean}: max |k.grad - face route| / bound = {(miss[bound > 0.0] / bound[bound > 0.0]).max():.3f}")
        assert (miss <= bound).all(), (name, np.unravel_index((miss - bound).argmax(), miss.shape), (miss - bound).max())
    # the three errors
    _, k, f, _ = _fields(n, 0.0, 195)
    g = boundary_for("dirichlet", n, 196)
    with Solver(n, box_dim=box_dim, b=B) as s:
        leaf = T(k).requires_grad_(True)
        u = autograd.solve_cells(s, T(f), None, leaf, boundary=T(g))
        s.set_cell_coefficients(None, leaf.detach())          # the same values: the version counts calls, it does not compare arrays
        assert "coefficients changed" in refused(u.sum().backward, kind=RuntimeError)
        assert refused(autograd.solve_cells, s, T(f), None, leaf, boundary=T(g).requires_grad_(True)).startswith("boundary: not differentiable")
        assert "did not converge" in refused(autograd.solve_cells, s, T(f), None, leaf, boundary=T(g), method="pcg", max_iter=1,
                                              kind=RuntimeError)       # one iteration does not reach rtol = 1e-10
        assert refused(autograd.solve_cells, s, T(f), None, leaf, mean="geometric").startswith("mean:")
    with Solver(n, box_dim=box_dim, bc=SOLVERS["corners"], b=B) as s:
        kap = T(kappa_for("corners", n)).requires_grad_(True)
        assert refused(autograd.solve_cells, s, T(f), None, T(k), robin=kap).startswith("robin: not differentiable")


def main():
    assert torch.cuda.is_available()
    H.load_driver().hpgmg_set_verbose(0)
    assert H.load_kernels().hpgmg_hip_set_device(torch.cuda.current_device()) == 0
    oracle = Backend.oracle().lib
    oracle.hpgmg_set_verbose(0)
    assert len(hip_runtimes_mapped()) == 1, hip_runtimes_mapped()
    dev = torch.device("cuda", torch.cuda.current_device())
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    tensors_equal_numpy(dev, T)
    autograd_equals_the_manual_composition(dev, T, oracle)
    print("torch worker ok")


if __name__ == "__main__":
    main()
