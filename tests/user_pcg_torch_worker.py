"""Child process of tests/test_gpu_user_pcg.py: torch first, then the project's libraries (one HIP runtime); method="pcg" on torch tensors must
equal the NumPy path bitwise, with and without boundary values and from a u0."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver, hip_runtimes_mapped  # noqa: E402
from user_problem_lib import random_coefficients  # noqa: E402


def main():
    assert torch.cuda.is_available()
    H.load_driver().hpgmg_set_verbose(0)
    assert H.load_kernels().hpgmg_hip_set_device(torch.cuda.current_device()) == 0
    assert len(hip_runtimes_mapped()) == 1, hip_runtimes_mapped()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 64
    coef = random_coefficients(n, "dirichlet", True, seed=66)
    rng = np.random.default_rng(4)
    f, g = rng.random((n, n, n)) - 0.5, rng.random((6, n, n)) - 0.5
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    with Solver(n, box_dim=32, smoother="cheby", a=1.0) as s:
        s.set_coefficients(*[T(c) for c in coef])
        for boundary in (None, g):
            u_h, info_h = s.solve(f, method="pcg", rtol=1e-9, boundary=boundary)
            u_d, info_d = s.solve(T(f), method="pcg", rtol=1e-9, boundary=None if boundary is None else T(boundary))
            assert isinstance(u_d, torch.Tensor) and u_d.device == dev
            assert info_h.converged and np.array_equal(u_d.cpu().numpy(), u_h)
            assert (info_d.residual, info_d.norm_f, info_d.vcycles) == (info_h.residual, info_h.norm_f, info_h.vcycles)
        start = u_h * (1.0 + 1e-3)
        w_h, again_h = s.solve(f, method="pcg", rtol=1e-9, boundary=g, u0=start)
        w_d, again_d = s.solve(T(f), method="pcg", rtol=1e-9, boundary=T(g), u0=T(start))
        assert again_h.converged and again_h.vcycles < info_h.vcycles
        assert np.array_equal(w_d.cpu().numpy(), w_h) and again_d.vcycles == again_h.vcycles
    print("torch worker ok")


if __name__ == "__main__":
    main()
