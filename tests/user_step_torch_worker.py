"""Child process of tests/test_gpu_user_step.py: torch first, then the project's libraries (one HIP runtime); Solver.start / step / rate on
torch tensors must equal the NumPy path bitwise, and a call that mixes the two kinds is refused by name."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver, StepInfo, hip_runtimes_mapped  # noqa: E402
from user_step_lib import B, data, initial, problem  # noqa: E402


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
    n, seed, dt = 32, 1700, 2e-3
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    for name, theta in (("corners", 0.5), ("periodic", 1.0)):
        bc, coef, kappa = problem(name, n, seed)
        seen = []
        for wrap in (lambda a: a, T):
            with Solver(n, box_dim=16, bc=bc, a=1.0, b=B) as s:
                s.set_coefficients(*[wrap(c) for c in coef], robin=wrap(kappa))
                f, g = data(name, n, seed, 0)
                s.start(wrap(initial(n, seed)), wrap(f), boundary=wrap(g), dt=dt, theta=theta)
                steps = []
                for k, step_dt in ((1, None), (2, dt / 4.0)):
                    f, g = data(name, n, seed, k)
                    info = s.step(wrap(f), boundary=wrap(g), dt=step_dt, rtol=1e-6)
                    assert isinstance(info, StepInfo)
                    u, w = s.get_solution(), s.rate()
                    steps.append((info, u, w))
                    if wrap is T:
                        into = torch.full((n, n, n), 7.0, dtype=torch.float64, device=dev)
                        assert s.rate(into) is into and np.array_equal(into.cpu().numpy(), w)
                        if g is not None:
                            assert refused(s.step, f, boundary=T(g)).startswith("boundary: a torch array among numpy arrays")
                            assert refused(s.step, T(f), boundary=g).startswith("boundary: a numpy array among torch arrays")
                        assert refused(s.start, T(initial(n, seed)), f, dt=dt).startswith("f: a numpy array among torch arrays")
                        assert refused(s.rate, torch.empty((n, n, n), dtype=torch.float32, device=dev)).startswith("out: dtype")
                        assert refused(s.step, T(f).float(), boundary=T(g)).startswith("f: dtype")
                        bad = f.copy()
                        bad[3, 4, 5] = np.nan
                        assert refused(s.step, T(bad), boundary=T(g)).startswith("f: holds a value that is not finite")
                        assert s.get_solution().tobytes() == u.tobytes() and s.rate().tobytes() == w.tobytes()      # the refusals changed nothing
                seen.append(steps)
        for (i_h, u_h, w_h), (i_d, u_d, w_d) in zip(*seen):
            assert i_h == i_d, (i_h, i_d)
            assert u_h.tobytes() == u_d.tobytes() and w_h.tobytes() == w_d.tobytes()
    print("torch worker ok")


if __name__ == "__main__":
    main()
