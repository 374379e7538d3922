"""Implicit time stepping on the MI355X: the HIP build (kernels/dense_step.hip, one launch per pass) equals the CPU oracle bit
for bit -- the state u, the rate array and every field a step reports -- over a march of three steps with changing f and g and a dt change at
the third, with arrays entering from the host (through the staging buffer) and from the device (in place); a refused step leaves the march
intact on the device too; torch tensors equal the NumPy path.

Shapes: N = 64 in boxes of 32 (2^3 boxes: every box on three walls), N = 48 in boxes of 16 (3^3 boxes: boxes on zero to three walls and,
periodic, the wrap) and N = 16 in boxes of 4 (rows shorter than a wave, 64 boxes).
"""
import os
import subprocess
import sys

import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays
from user_step_lib import march

pytestmark = pytest.mark.gpu

DTS = [2e-3, 2e-3, 5e-4]                 # "as before" at the second step, a change at the third
RTOL = 1e-6


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


_oracle = {}


def _reference(oracle, n, box_dim, name, theta, spoil=None):
    """The oracle's march, computed once per configuration and shared by the host and device cases."""
    key = (n, box_dim, name, theta, spoil)
    if key not in _oracle:
        _oracle[key] = march(oracle, n, box_dim, name, 1500 + n, theta, DTS, RTOL, spoil=spoil)
    return _oracle[key]


def _same(got, ref):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref), start=1):
        if r[0] == "refused":
            assert g == r, k
            continue
        assert g[0] == r[0] == H.USER_OK, k
        assert g[1].tobytes() == r[1].tobytes(), f"u after step {k}"
        assert g[2].tobytes() == r[2].tobytes(), f"rate after step {k}"
        assert g[3] == r[3] and g[4] == r[4], (k, g[3:], r[3:])
        assert g[4] == abs(g[2]).max(), k


SHAPES = [(64, 32), (48, 16), (16, 4)]
WALLS = ["dirichlet", "periodic", "corners", "robin"]
# every shape and wall configuration with theta = 1/2, and theta = 1 on every wall configuration at the shape with boxes on 0 to 3 walls and at the
# one with short rows; each from host and from device arrays (the oracle's march is computed once per configuration)
CASES = [(n, box_dim, name, 0.5, entry) for n, box_dim in SHAPES for name in WALLS for entry in ("host", "device")]
CASES += [(n, box_dim, name, 1.0, entry) for n, box_dim in SHAPES[1:] for name in WALLS for entry in ("host", "device")]


@pytest.mark.parametrize("n,box_dim,name,theta,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, name, theta, entry):
    hip, oracle, K = libs
    ref = _reference(oracle, n, box_dim, name, theta)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = march(hip, n, box_dim, name, 1500 + n, theta, DTS, RTOL, device=D)
    finally:
        if D:
            D.free()
    _same(got, ref)


@pytest.mark.parametrize("what,entry", [("f", "device"), ("g", "host"), ("g", "device")])
def test_a_refused_step_leaves_the_march_intact(libs, what, entry):
    hip, oracle, K = libs
    n, box_dim, name = 48, 16, "corners"
    plain = _reference(oracle, n, box_dim, name, 0.5)
    ref = _reference(oracle, n, box_dim, name, 0.5, spoil=(2, what))
    assert ref[1] == ("refused", H.USER_NOT_FINITE) and len(ref) == len(plain) + 1
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = march(hip, n, box_dim, name, 1500 + n, 0.5, DTS, RTOL, device=D, spoil=(2, what))
    finally:
        if D:
            D.free()
    _same(got, ref)
    _same(got[:1] + got[2:], plain)                             # the good steps are those of the undisturbed march


def test_torch_tensors(libs):
    """A child process that imports torch first: start / step / rate on tensors equal the NumPy path bitwise, and mixed kinds are refused."""
    worker = os.path.join(ROOT, "tests", "user_step_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
