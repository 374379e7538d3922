"""Child process of tests/test_gpu_user_problem.py: torch first, then the project's libraries (one HIP runtime); the user-problem API on
torch tensors must equal the NumPy path bitwise and fill out= in place."""
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
    runtimes = hip_runtimes_mapped()
    assert len(runtimes) == 1, runtimes
    dev = torch.device("cuda", torch.cuda.current_device())
    for bc, a, smoother in (("dirichlet", 1.0, "cheby"), ("periodic", 0.0, "gsrb")):
        n = 64
        coef = random_coefficients(n, bc, a != 0.0, seed=64)
        rng = np.random.default_rng(1)
        f, x = rng.random((n, n, n)) - 0.5, rng.random((n, n, n))
        with Solver(n, box_dim=32, bc=bc, smoother=smoother, a=a) as s:
            s.set_coefficients(*coef)
            u_h, info_h = s.solve(f, method="mg", rtol=1e-10)
            y_h = s.apply(x)
            tc = [None if c is None else torch.from_numpy(c).to(dev) for c in coef]
            s.set_coefficients(*tc)
            out = torch.full((n, n, n), -7.0, dtype=torch.float64, device=dev)
            ptr = out.data_ptr()
            u_d, info_d = s.solve(torch.from_numpy(f).to(dev), method="mg", rtol=1e-10, out=out)
            assert u_d is out and out.data_ptr() == ptr
            y_d = s.apply(torch.from_numpy(x).to(dev))
            assert isinstance(y_d, torch.Tensor) and y_d.device == dev
            assert np.array_equal(u_d.cpu().numpy(), u_h), bc
            assert np.array_equal(y_d.cpu().numpy(), y_h), bc
            assert (info_d.residual, info_d.vcycles) == (info_h.residual, info_h.vcycles)
            try:
                s.apply(torch.from_numpy(x).to(dev).float())
                raise AssertionError("a float32 tensor was accepted")
            except ValueError as e:
                assert "x: dtype" in str(e)
    print("torch worker ok")


if __name__ == "__main__":
    main()
