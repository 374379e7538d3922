"""Child process of tests/test_gpu_user_wave.py: torch first, then the project's libraries (one HIP runtime); Solver.wave_start / wave_step / velocity /
acceleration on torch tensors must equal the NumPy path bitwise, and a call that mixes the two kinds is refused by name."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver, WaveInfo, hip_runtimes_mapped  # noqa: E402
from user_step_lib import B, data, initial, problem  # noqa: E402
from user_wave_lib import velocity0  # noqa: E402


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
    for name, sigma in (("corners", 0.3), ("periodic", 0.0)):
        bc, coef, kappa = problem(name, n, seed)
        seen = []
        for wrap in (lambda a: a, T):
            with Solver(n, box_dim=16, bc=bc, a=1.0, b=B) as s:
                s.set_coefficients(*[wrap(c) for c in coef], robin=wrap(kappa))
                f, g = data(name, n, seed, 0)
                info = s.wave_start(wrap(initial(n, seed)), wrap(velocity0(n, seed)), wrap(f), boundary=wrap(g), dt=dt, damping=sigma)
                steps = [(info, s.get_solution(), s.velocity(), s.acceleration())]
                for k, step_dt in ((1, None), (2, dt / 4.0)):
                    f, g = data(name, n, seed, k)
                    info = s.wave_step(wrap(f), boundary=wrap(g), dt=step_dt, rtol=1e-6)
                    assert isinstance(info, WaveInfo) and info.energy == info.kinetic + info.potential
                    u, v, q = s.get_solution(), s.velocity(), s.acceleration()
                    steps.append((info, u, v, q))
                    if wrap is T:
                        into = torch.full((n, n, n), 7.0, dtype=torch.float64, device=dev)
                        assert s.velocity(into) is into and np.array_equal(into.cpu().numpy(), v)
                        assert s.acceleration(into) is into and np.array_equal(into.cpu().numpy(), q)
                        if g is not None:
                            assert refused(s.wave_step, f, boundary=T(g)).startswith("boundary: a torch array among numpy arrays")
                            assert refused(s.wave_step, T(f), boundary=g).startswith("boundary: a numpy array among torch arrays")
                        assert refused(s.wave_start, T(initial(n, seed)), velocity0(n, seed), T(f), dt=dt).startswith("v: a numpy array among torch arrays")
                        assert refused(s.velocity, torch.empty((n, n, n), dtype=torch.float32, device=dev)).startswith("out: dtype")
                        assert refused(s.wave_step, T(f).float(), boundary=T(g)).startswith("f: dtype")
                        bad = f.copy()
                        bad[3, 4, 5] = np.nan
                        assert refused(s.wave_step, T(bad), boundary=T(g)).startswith("f: holds a value that is not finite")
                        assert s.get_solution().tobytes() == u.tobytes() and s.velocity().tobytes() == v.tobytes() and s.acceleration().tobytes() == q.tobytes()
                seen.append(steps)
        for (i_h, u_h, v_h, q_h), (i_d, u_d, v_d, q_d) in zip(*seen):
            assert i_h == i_d, (i_h, i_d)
            assert u_h.tobytes() == u_d.tobytes() and v_h.tobytes() == v_d.tobytes() and q_h.tobytes() == q_d.tobytes()
    print("torch worker ok")


if __name__ == "__main__":
    main()
