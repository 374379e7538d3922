"""Child process of tests/test_gpu_user_sensitivity.py: torch first, then the project's libraries (one HIP runtime).  Solver.sensitivity on torch
tensors must equal the NumPy path bitwise and write out= in place; hpgmg_amd.autograd.solve must give, bitwise, the gradients of the manual
composition (lam for f, -sensitivity(u, lam, boundary=g) for the coefficients) on a second solver and on the CPU oracle; its three errors raise."""
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
from user_flux_lib import SOLVERS, boundary_for, kappa_for  # noqa: E402
from user_problem_lib import random_coefficients  # noqa: E402

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


def tensors_equal_numpy(dev, T):
    n = 64
    for name, a in (("corners", 1.3), ("periodic", 0.0)):
        bc = "periodic" if name == "periodic" else "dirichlet"
        coef = random_coefficients(n, bc, a != 0.0, seed=81)
        kappa, g = kappa_for(name, n), boundary_for(name, n, 82)
        rng = np.random.default_rng(83)
        u, lam = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5
        with Solver(n, box_dim=32, bc=SOLVERS[name], a=a, b=B) as s:
            s.set_coefficients(*coef, robin=kappa)
            host = s.sensitivity(u, lam, boundary=g)
            got = s.sensitivity(T(u), T(lam), boundary=T(g))
            assert (got[0] is None) == (a == 0.0)
            for q_h, q_d in zip(host, got):
                assert q_d is None or (isinstance(q_d, torch.Tensor) and q_d.device == dev and q_d.dtype == torch.float64)
                assert same(q_d, q_h)
            into = tuple(None if q is None else torch.full_like(q, float("nan")) for q in got)
            back = s.sensitivity(T(u), T(lam), boundary=T(g), out=into)
            assert all(x is y for x, y in zip(back, into))
            for q_h, q_d in zip(host, into):
                assert same(q_d, q_h)
            assert refused(s.sensitivity, T(u), lam).startswith("lam: a numpy array among torch arrays")
            assert refused(s.sensitivity, u, T(lam)).startswith("lam: a torch array among numpy arrays")
            assert refused(s.sensitivity, T(u), T(lam), out=host).startswith(("out[0]: a numpy", "out[1]: a numpy"))
            assert refused(s.sensitivity, T(u), T(lam), out=(got[0], got[1], got[2], got[3].float())).startswith("out[3]: dtype")
            if g is not None:
                assert refused(s.sensitivity, T(u), T(lam), boundary=g).startswith("boundary: a numpy array among torch arrays")
                bad = g.copy()
                bad[4, 5, 6] = np.nan
                assert refused(s.sensitivity, T(u), T(lam), boundary=T(bad)).startswith("boundary:")


def autograd_equals_the_manual_composition(dev, T, oracle):
    n, box_dim, rtol = 32, 16, 1e-10
    for name, a in (("dirichlet", 1.3), ("corners", 0.0)):
        coef = random_coefficients(n, "dirichlet", a != 0.0, seed=91)
        kappa, g = kappa_for(name, n), boundary_for(name, n, 92)
        rng = np.random.default_rng(93)
        f, w = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5
        leaves = [None if c is None else T(c).requires_grad_(True) for c in coef]
        tf = T(f).requires_grad_(True)
        with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B) as s:
            u = autograd.solve(s, tf, *leaves, boundary=T(g), robin=None if kappa is None else T(kappa), method="mg", rtol=rtol)
            assert isinstance(u, torch.Tensor) and u.requires_grad
            (T(w) * u).sum().backward()                  # grad_u is exactly w
            assert same(s.get_solution(torch.empty_like(u)), tf.grad.cpu().numpy())      # backward leaves lam as the last solution
        grads = [tf.grad] + [None if x is None else x.grad for x in leaves]
        # the manual composition on a second solver of the product, from tensors, and on the oracle, from NumPy arrays
        for lib, put in ((None, T), (oracle, lambda v: v)):
            with Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=B, lib=lib) as m:
                m.set_coefficients(*[None if c is None else put(c) for c in coef], robin=None if kappa is None else put(kappa))
                u2, info = m.solve(put(f), method="mg", rtol=rtol, boundary=put(g))
                assert info.converged
                lam, info = m.solve(put(w), method="mg", rtol=rtol)
                assert info.converged
                G = m.sensitivity(u2, lam, boundary=put(g))
            numpy_of = (lambda v: v.cpu().numpy()) if lib is None else (lambda v: v)
            assert same(u.detach(), numpy_of(u2)), (name, "u")
            assert same(grads[0], numpy_of(lam)), (name, "f")
            for slot, (got, ref) in enumerate(zip(grads[1:], G)):
                assert same(got, None if ref is None else -numpy_of(ref)), (name, slot)
    # the three errors
    coef = random_coefficients(n, "dirichlet", False, seed=95)
    g = boundary_for("dirichlet", n, 96)
    f = np.random.default_rng(97).random((n, n, n)) - 0.5
    with Solver(n, box_dim=box_dim, b=B) as s:
        leaves = [T(c).requires_grad_(True) for c in coef[1:]]
        u = autograd.solve(s, T(f), None, *leaves, boundary=T(g))
        s.set_coefficients(None, *[x.detach() for x in leaves])          # the same values: the version counts calls, it does not compare arrays
        assert "coefficients changed" in refused(u.sum().backward, kind=RuntimeError)
        assert refused(autograd.solve, s, T(f), None, *leaves, boundary=T(g).requires_grad_(True)).startswith("boundary: not differentiable")
        assert "did not converge" in refused(autograd.solve, s, T(f), None, *leaves, boundary=T(g), method="pcg", max_iter=1,
                                              kind=RuntimeError)       # one iteration does not reach rtol = 1e-10
    with Solver(n, box_dim=box_dim, bc=SOLVERS["corners"], b=B) as s:
        kap = T(kappa_for("corners", n)).requires_grad_(True)
        assert refused(autograd.solve, s, T(f), None, *[T(c) for c in coef[1:]], robin=kap).startswith("robin: not differentiable")


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
