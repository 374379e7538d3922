"""Child process of tests/test_gpu_user_robin.py: torch first, then the project's libraries (one HIP runtime); a solver with Robin walls on
torch tensors must equal the NumPy path bitwise, and a call that mixes the two kinds is refused by name."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver, hip_runtimes_mapped  # noqa: E402
from user_problem_lib import random_coefficients  # noqa: E402
from user_robin_lib import ALL, CORNERS, kappa_of  # noqa: E402


def refused(call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except ValueError as e:
        return str(e)
    raise AssertionError("mixed NumPy / torch arrays were accepted")


def main():
    assert torch.cuda.is_available()
    H.load_driver().hpgmg_set_verbose(0)
    assert H.load_kernels().hpgmg_hip_set_device(torch.cuda.current_device()) == 0
    assert len(hip_runtimes_mapped()) == 1, hip_runtimes_mapped()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 64
    rng = np.random.default_rng(3)
    f, x, g = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)), rng.random((6, n, n)) - 0.5
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    for faces, a in ((CORNERS, 1.0), (ALL, 0.0)):
        coef = random_coefficients(n, "dirichlet", a != 0.0, seed=67)
        kappa = kappa_of(n, faces)
        with Solver(n, box_dim=32, bc=faces, smoother="cheby", a=a) as s:
            s.set_coefficients(*coef, robin=kappa)
            host = [s.solve(f, method=m, boundary=g) for m in ("fmg", "mg")] + [s.solve(f)]
            y_h = s.apply(x, boundary=g)
            assert refused(s.set_coefficients, *coef, robin=T(kappa)).startswith("robin: a torch array among numpy arrays")
            assert refused(s.set_coefficients, *[T(c) for c in coef], robin=kappa).startswith("robin: a numpy array among torch arrays")
            s.set_coefficients(*[T(c) for c in coef], robin=T(kappa))
            dev_out = [s.solve(T(f), method=m, boundary=T(g)) for m in ("fmg", "mg")] + [s.solve(T(f))]
            for (u_h, i_h), (u_d, i_d) in zip(host, dev_out):
                assert isinstance(u_d, torch.Tensor) and u_d.device == dev
                assert np.array_equal(u_d.cpu().numpy(), u_h)
                assert (i_d.residual, i_d.norm_f, i_d.vcycles, i_d.mean_shift) == (i_h.residual, i_h.norm_f, i_h.vcycles, i_h.mean_shift)
            assert np.array_equal(s.apply(T(x), boundary=T(g)).cpu().numpy(), y_h)
            bad = kappa.copy()
            bad[faces.index("convective"), 3, 4] = -1.0
            assert refused(s.set_coefficients, *[T(c) for c in coef], robin=T(bad)).startswith("robin:")
            s.set_coefficients(*[T(c) for c in coef], robin=[0.5] * 6)             # six numbers go to the tensors' device
            u_six, _ = s.solve(T(f), boundary=T(g))
            s.set_coefficients(*coef, robin=[0.5] * 6)
            assert np.array_equal(u_six.cpu().numpy(), s.solve(f, boundary=g)[0])
    print("torch worker ok")


if __name__ == "__main__":
    main()
