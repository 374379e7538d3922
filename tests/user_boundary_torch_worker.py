"""Child process of tests/test_gpu_user_boundary.py: torch first, then the project's libraries (one HIP runtime); boundary= on torch tensors
must equal the NumPy path bitwise."""
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
    coef = random_coefficients(n, "dirichlet", True, seed=65)
    rng = np.random.default_rng(2)
    f, x, g = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)), rng.random((6, n, n)) - 0.5
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    with Solver(n, box_dim=32, smoother="cheby", a=1.0) as s:
        s.set_coefficients(*coef)
        s.set_coefficients(*[T(c) for c in coef])
        for method in ("fmg", "mg"):
            u_h, info_h = s.solve(f, method=method, boundary=g)
            u_d, info_d = s.solve(T(f), method=method, boundary=T(g))
            assert isinstance(u_d, torch.Tensor) and u_d.device == dev
            assert np.array_equal(u_d.cpu().numpy(), u_h), method
            assert (info_d.residual, info_d.norm_f, info_d.vcycles) == (info_h.residual, info_h.norm_f, info_h.vcycles)
        y_h = s.apply(x, boundary=g)
        y_d = s.apply(T(x), boundary=T(g))
        assert np.array_equal(y_d.cpu().numpy(), y_h)
        try:
            s.solve(T(f), boundary=g)
            raise AssertionError("a NumPy boundary among tensors was accepted")
        except ValueError as e:
            assert str(e).startswith("boundary:"), e
    print("torch worker ok")


if __name__ == "__main__":
    main()
