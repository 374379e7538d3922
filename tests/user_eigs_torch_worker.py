"""Child process of tests/test_gpu_user_eigs.py: torch first, then the project's libraries (one HIP runtime).  Solver.eigs with a start block and an
output block that are GPU tensors must give the bytes of the NumPy path, write out= in place and return a tensor when only x0 is one; arrays of two
kinds in one call are refused."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
import user_eigs_lib as E  # noqa: E402
from hpgmg_amd.problem import Solver, hip_runtimes_mapped  # noqa: E402


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
    T = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    n, k = 16, 3
    x0 = np.random.default_rng(21).random((k + 2, n, n, n)) - 0.5
    for name in ("corners", "poisson"):
        with Solver(n, box_dim=8, bc=E.bc_of(name), a=E.CASES[name][1], b=E.B) as s:
            E.set_case(s, name, n)
            lam, modes, info = s.eigs(k, x0=x0)
            assert isinstance(modes, np.ndarray) and info.converged
            into = torch.full((k, n, n, n), float("nan"), dtype=torch.float64, device=dev)
            lam_t, modes_t, info_t = s.eigs(k, x0=T(x0), out=into)
            assert modes_t is into and into.cpu().numpy().tobytes() == modes.tobytes() and lam_t.tobytes() == lam.tobytes()
            assert info_t.iterations == info.iterations and info_t.residuals.tobytes() == info.residuals.tobytes()
            lam_d, modes_d, _ = s.eigs(k, x0=T(x0))                       # out=None follows x0's kind
            assert isinstance(modes_d, torch.Tensor) and modes_d.device == dev and modes_d.cpu().numpy().tobytes() == modes.tobytes()
            lam_n, modes_n, _ = s.eigs(k, out=into)                       # the default start, into a tensor
            assert modes_n is into and into.cpu().numpy().tobytes() == s.eigs(k)[1].tobytes()
            assert refused(s.eigs, k, x0=T(x0), out=np.empty((k, n, n, n))).startswith("out: a numpy array among torch arrays")
            assert refused(s.eigs, k, x0=x0, out=into).startswith("out: a torch array among numpy arrays")
            assert refused(s.eigs, k, out=into.float()).startswith("out: dtype")
    print("torch worker ok")


if __name__ == "__main__":
    main()
