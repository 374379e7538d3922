"""Child process of tests/test_gpu_user_step.py: the waves per workgroup of the sweep-pair kernel are chosen once per process (HPGMG_TUNE_PAIR_NW),
so the march at N = 128 in boxes of 64 with a wave count that forms Dinv in registers runs here: once with the switch on and once with it
off, one JSON line each with the digests of the steps (user_step_lib.digests) and, per step, how many sweep-pair launches there were and how
many of them formed Dinv."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402,F401  (the OpenMP environment of the suite, before any runtime loads)

import hpgmg_amd as H  # noqa: E402
from user_step_lib import digests, march  # noqa: E402


def main():
    n, box_dim, name, theta, rtol = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], float(sys.argv[4]), float(sys.argv[5])
    dts = [float(x) for x in sys.argv[6:]]
    lib, K = H.load_driver(), H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    lib.hpgmg_set_verbose(0)
    lib.hpgmg_set_pair_form_dinv.argtypes = [ctypes.c_int]
    lib.hpgmg_pair_formed_dinv_launches.restype = ctypes.c_longlong

    def counters():
        pairs = (ctypes.c_longlong * 2)()
        K.hpgmg_hip_pair_launch_counts(pairs)
        return pairs[0], lib.hpgmg_pair_formed_dinv_launches()

    for switch in (1, 0):
        lib.hpgmg_set_pair_form_dinv(switch)
        rise = {}

        def watch(k, done):
            now = counters()
            rise[k] = [a - b for a, b in zip(now, rise[k])] if done else now

        steps = march(lib, n, box_dim, name, 1500 + n, theta, dts, rtol, watch=watch)
        print("MARCH " + json.dumps({"switch": switch, "digests": digests(steps), "pairs": [rise[k][0] for k in sorted(rise)],
                                     "formed": [rise[k][1] for k in sorted(rise)]}), flush=True)
    lib.hpgmg_set_pair_form_dinv(1)


if __name__ == "__main__":
    main()
