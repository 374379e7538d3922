"""One rank of tests/test_gpu_ca_bottom.py's multi-rank job: tests/multirank_worker.py with the bottom solver (and, optionally, the U-cycle ladder)
chosen before the solver is built.  HPGMG_TEST_BOTTOM_SOLVER = one of hpgmg_amd.BOTTOM_*, HPGMG_TEST_UCYCLES = 1 for -DUSE_UCYCLES."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multirank_worker  # noqa: E402
from hpgmg_testlib import Backend  # noqa: E402

_configure = Backend.configure


def configure(self, **kw):      # the worker configures once, right before hpgmg_solver_create (MGBuild sizes the bottom level's work vectors)
    self.lib.hpgmg_set_bottom_solver(int(os.environ["HPGMG_TEST_BOTTOM_SOLVER"]))
    self.lib.hpgmg_set_ucycles(int(os.environ.get("HPGMG_TEST_UCYCLES", "0")))
    return _configure(self, **kw)


Backend.configure = configure

if __name__ == "__main__":
    multirank_worker.main()
