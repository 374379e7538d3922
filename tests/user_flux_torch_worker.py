"""Child process of tests/test_gpu_user_flux.py: torch first, then the project's libraries (one HIP runtime); Solver.flux and Solver.wall_flux
on torch tensors must equal the NumPy path bitwise, and a call that mixes the two kinds is refused by name."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver, hip_runtimes_mapped  # noqa: E402
from user_flux_lib import SOLVERS, boundary_for, kappa_for  # noqa: E402
from user_problem_lib import random_coefficients  # noqa: E402


def refused(call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except ValueError as e:
        return str(e)
    raise AssertionError("the call was accepted")


def main():
    assert torch.cuda.is_available()
    H.load_driver().hpgmg_set_verbose(0)
    assert H.load_kernels().hpgmg_hip_set_device(torch.cuda.current_device()) == 0
    assert len(hip_runtimes_mapped()) == 1, hip_runtimes_mapped()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 64
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    for name, a in (("corners", 1.0), ("periodic", 0.0)):
        bc = "periodic" if name == "periodic" else "dirichlet"
        coef = random_coefficients(n, bc, a != 0.0, seed=71)
        kappa, g = kappa_for(name, n), boundary_for(name, n, 72)
        u = np.random.default_rng(73).random((n, n, n)) - 0.5
        with Solver(n, box_dim=32, bc=SOLVERS[name], a=a) as s:
            s.set_coefficients(*coef, robin=kappa)
            host = s.flux(u, boundary=g)
            got = s.flux(T(u), boundary=T(g))
            for q_h, q_d in zip(host, got):
                assert isinstance(q_d, torch.Tensor) and q_d.device == dev and q_d.dtype == torch.float64
                assert np.array_equal(q_d.cpu().numpy(), q_h)
            into = tuple(torch.full_like(q, 7.0) for q in got)
            assert s.flux(T(u), boundary=T(g), out=into)[0] is into[0]
            for q_h, q_d in zip(host, into):
                assert np.array_equal(q_d.cpu().numpy(), q_h)
            assert refused(s.flux, T(u), out=host).startswith("out[0]: a numpy array among torch arrays")
            assert refused(s.flux, u, out=got).startswith("out[0]: a torch array among numpy arrays")
            assert refused(s.flux, T(u), out=(got[0], got[1], got[2].float())).startswith("out[2]: dtype")
            if g is not None:
                assert refused(s.flux, T(u), boundary=g).startswith("boundary: a numpy array among torch arrays")
                bad = g.copy()
                bad[4, 5, 6] = np.nan
                assert refused(s.flux, T(u), boundary=T(bad)).startswith("boundary:")
                w_h, w_d = s.wall_flux(host), s.wall_flux(got)
                assert isinstance(w_d, torch.Tensor) and w_d.is_contiguous() and tuple(w_d.shape) == (6, n, n)
                assert np.array_equal(w_d.cpu().numpy(), w_h)
                assert refused(s.wall_flux, (got[0], host[1], host[2])).startswith("fluxes[1]: a numpy array among torch arrays")
            else:
                assert refused(s.wall_flux, got).startswith("fluxes:")
    print("torch worker ok")


if __name__ == "__main__":
    main()
