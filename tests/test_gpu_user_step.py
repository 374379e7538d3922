"""Implicit time stepping on the MI355X: the HIP build (kernels/dense_step.hip, one launch per pass) equals the CPU oracle bit
for bit -- the state u, the rate array and every field a step reports -- over a march of three steps with changing f and g and a dt change at
the third, with arrays entering from the host (through the staging buffer) and from the device (in place); a refused step leaves the march
intact on the device too; torch tensors equal the NumPy path.

Shapes: N = 64 in boxes of 32 (2^3 boxes: every box on three walls), N = 48 in boxes of 16 (3^3 boxes: boxes on zero to three walls and,
periodic, the wrap) and N = 16 in boxes of 4 (rows shorter than a wave, 64 boxes).

And where the product's path changes: N = 128 in boxes of 64, the smallest level that smooths as sweep pairs (kernels/pair.hip), against the oracle
-- with Dinv formed in registers after the dt change (a worker process with a wave count that forms), and with the fp32 coefficient copies,
whose Dinv every set_shift changes --, and N = 256 in boxes of 128, the README's example and the smallest level with packed edge coefficients,
against the same march without the fused sweeps.  Each state is shown to be reached by the library's own counters.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays
from user_lifecycle_lib import coefficients
from user_step_lib import digests, march

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


# ---------------------------------------------------------------- the sweep-pair level: N = 128 in boxes of 64
PAIR_N, PAIR_BOX = 128, 64


def _pair_launches(K):
    out = (ctypes.c_longlong * 2)()
    K.hpgmg_hip_pair_launch_counts(out)
    return out[0]


def _rises(read):
    """(watch of march(), {step: rise of read() over that step's hpgmg_user_step call})"""
    rise = {}

    def watch(k, done):
        rise[k] = read() - rise[k] if done else read()
    return watch, rise


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", ["dirichlet", "robin"])
def test_sweep_pair_level_equals_the_oracle(libs, name, entry):
    """The finest level smooths as sweep pairs, whose launches read Dinv or form it under a record that the set_shift of start() and of the dt
    change at the third step must re-establish for the new a."""
    hip, oracle, K = libs
    ref = _reference(oracle, PAIR_N, PAIR_BOX, name, 0.5)
    watch, pairs = _rises(lambda: _pair_launches(K))
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = march(hip, PAIR_N, PAIR_BOX, name, 1500 + PAIR_N, 0.5, DTS, RTOL, device=D, watch=watch)
    finally:
        if D:
            D.free()
    _same(got, ref)
    assert sorted(pairs) == [1, 2, 3] and all(v > 0 for v in pairs.values()), f"sweep-pair launches per step: {pairs}"


@pytest.mark.parametrize("nw", [10])
def test_sweep_pair_level_forms_dinv_after_the_dt_change(libs, nw):
    """A worker process with 10 waves per workgroup, which form Dinv in registers where the level's record allows: the step after the dt change
    forms it again, for the new a, and computes the oracle's bits; so does the switch off, which forms nothing."""
    _, oracle, _ = libs
    ref = digests(_reference(oracle, PAIR_N, PAIR_BOX, "dirichlet", 0.5))
    worker = os.path.join(ROOT, "tests", "user_step_pair_worker.py")
    cmd = [sys.executable, worker, str(PAIR_N), str(PAIR_BOX), "dirichlet", "0.5", repr(RTOL)] + [repr(dt) for dt in DTS]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, HPGMG_TUNE_PAIR_NW=str(nw)))
    assert out.returncode == 0, out.stdout[-800:] + out.stderr[-800:]
    on, off = [json.loads(line[6:]) for line in out.stdout.splitlines() if line.startswith("MARCH ")]
    print(on["pairs"], on["formed"], off["pairs"], off["formed"])
    assert (on["switch"], off["switch"]) == (1, 0)
    assert on["digests"] == ref, "Dinv formed in registers: not the oracle's march"
    assert off["digests"] == ref, "Dinv read: not the oracle's march"
    assert all(v > 0 for v in on["pairs"] + off["pairs"])
    assert all(v > 0 for v in on["formed"]), f"formed-Dinv launches per step {on['formed']}: the step after the dt change is the third"
    assert off["formed"] == [0, 0, 0]


def test_sweep_pair_level_with_fp32_coefficient_copies(libs):
    """Smoother precision 32 on both libraries: the sweep pairs read fp32 copies of the coefficients, Dinv among them, which start() and the dt
    change of the third step make stale.  Every step smooths in fp32, as often as the oracle, and gives its bits."""
    hip, oracle, K = libs
    for lib in (hip, oracle):
        lib.hpgmg_set_smoother_precision.argtypes = [ctypes.c_int]
        lib.hpgmg_fp32_pair_smooths.restype = ctypes.c_longlong
    smooths, runs = {}, {}
    try:
        for lib in (oracle, hip):
            lib.hpgmg_set_smoother_precision(32)
            watch, smooths[lib] = _rises(lib.hpgmg_fp32_pair_smooths)
            runs[lib] = march(lib, PAIR_N, PAIR_BOX, "dirichlet", 1500 + PAIR_N, 0.5, DTS, RTOL, watch=watch)
    finally:
        for lib in (hip, oracle):
            lib.hpgmg_set_smoother_precision(64)
    print(smooths[hip], smooths[oracle])
    assert sorted(smooths[hip]) == [1, 2, 3] and all(v > 0 for v in smooths[hip].values()), smooths[hip]
    assert smooths[hip] == smooths[oracle]
    _same(runs[hip], runs[oracle])
    plain = _reference(oracle, PAIR_N, PAIR_BOX, "dirichlet", 0.5)
    assert runs[hip][0][1].tobytes() != plain[0][1].tobytes(), "precision 32 changed nothing"


# ---------------------------------------------------------------- packed edge coefficients: N = 256 in boxes of 128, the README's example
def test_packed_edge_coefficients_through_a_march(libs):
    """Convective walls, three steps with the dt change, arrays in device memory.  The reference is the same march without the fused sweeps, which
    use neither pairs nor packs: the path the other tests hold to the oracle (tests/test_gpu_user_lifecycle.py does the same for solves)."""
    hip, _, K = libs
    hip.hpgmg_set_fused_sweeps.argtypes = [ctypes.c_int]
    n, box_dim = 256, 128
    coef = coefficients((n, box_dim, "dirichlet", "cheby", 1.0), 2560)      # plain random fields: only bits are compared
    runs, pairs = {}, {}
    D = DeviceArrays(K)
    try:
        for fused in (0, 1):
            hip.hpgmg_set_fused_sweeps(fused)
            watch, pairs[fused] = _rises(lambda: _pair_launches(K))
            runs[fused] = march(hip, n, box_dim, "robin", 1500 + n, 0.5, DTS, RTOL, device=D, watch=watch, coef=coef)
    finally:
        hip.hpgmg_set_fused_sweeps(1)
        D.free()
    print(pairs)
    _same(runs[1], runs[0])                                            # with it: info.rate == abs(rate array).max() at every step
    assert all(v > 0 for v in pairs[1].values()) and sorted(pairs[1]) == [1, 2, 3], pairs[1]
    assert all(v == 0 for v in pairs[0].values()) and sorted(pairs[0]) == [1, 2, 3], pairs[0]
