"""The Newmark march on the MI355X: the HIP build (kernels/dense_wave.hip, one launch per pass and a fold launch for the two sums)
equals the CPU oracle bit for bit -- u, v, the acceleration and every field a call reports, the energies among them -- from wave_start over three steps
with changing f and g and a dt change at the third, with arrays entering from the host (through the staging buffer) and from the device (in place); a
refused step leaves the march intact on the device too; torch tensors equal the NumPy path.

Shapes: N = 64 in boxes of 32 (2^3 boxes: every box on three walls; two segments, four column blocks), N = 48 in boxes of 16 (3^3 boxes: boxes on zero to
three walls and, periodic, the wrap) and N = 16 in boxes of 4 (16 live columns of 256, 64 boxes).
"""
import os
import subprocess
import sys

import pytest

import hpgmg_amd as H
import user_wave_lib as W
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays

pytestmark = pytest.mark.gpu

DTS = [2e-3, 2e-3, 5e-4]                 # "as before" at the second step, a change at the third
RTOL = 1e-6
UNDAMPED, DAMPED = (0.25, 0.5, 0.0), (0.3025, 0.6, 0.2)


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


_oracle = {}


def _reference(oracle, n, box_dim, name, rule, spoil=None):
    """The oracle's march, computed once per configuration and shared by the host and device cases."""
    key = (n, box_dim, name, rule, spoil)
    if key not in _oracle:
        _oracle[key] = W.march(oracle, n, box_dim, name, 1500 + n, rule, DTS, RTOL, spoil=spoil)
    return _oracle[key]


SHAPES = [(64, 32), (48, 16), (16, 4)]
WALLS = ["dirichlet", "periodic", "corners", "robin"]
# every shape and wall configuration with sigma > 0 (and a rule off the default), and the default undamped rule on every wall configuration at the shape
# with boxes on 0 to 3 walls and at the one with short rows; each from host and from device arrays
CASES = [(n, box_dim, name, DAMPED, entry) for n, box_dim in SHAPES for name in WALLS for entry in ("host", "device")]
CASES += [(n, box_dim, name, UNDAMPED, entry) for n, box_dim in SHAPES[1:] for name in WALLS for entry in ("host", "device")]


@pytest.mark.parametrize("n,box_dim,name,rule,entry", CASES, ids=lambda v: "sigma%g" % v[2] if isinstance(v, tuple) else str(v))
def test_hip_equals_oracle(libs, n, box_dim, name, rule, entry):
    hip, oracle, K = libs
    ref = _reference(oracle, n, box_dim, name, rule)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = W.march(hip, n, box_dim, name, 1500 + n, rule, DTS, RTOL, device=D)
    finally:
        if D:
            D.free()
    W.same_march(got, ref)
    assert all(step[4][3] > 0 for step in got[1:]) and got[0][4][3] == 0          # V-cycles in every step, none at the start


@pytest.mark.parametrize("what,entry", [("f", "device"), ("g", "host"), ("g", "device")])
def test_a_refused_step_leaves_the_march_intact(libs, what, entry):
    hip, oracle, K = libs
    n, box_dim, name = 48, 16, "corners"
    plain = _reference(oracle, n, box_dim, name, DAMPED)
    ref = _reference(oracle, n, box_dim, name, DAMPED, spoil=(2, what))
    assert ref[2] == ("refused", H.USER_NOT_FINITE) and len(ref) == len(plain) + 1
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = W.march(hip, n, box_dim, name, 1500 + n, DAMPED, DTS, RTOL, device=D, spoil=(2, what))
    finally:
        if D:
            D.free()
    W.same_march(got, ref)
    W.same_march(got[:2] + got[3:], plain)                      # the good steps are those of the undisturbed march


def test_torch_tensors(libs):
    """A child process that imports torch first: wave_start / wave_step / velocity / acceleration on tensors equal the NumPy path bitwise, and mixed kinds
    are refused."""
    worker = os.path.join(ROOT, "tests", "user_wave_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
