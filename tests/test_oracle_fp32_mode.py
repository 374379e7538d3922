"""The CPU oracle's fp32-coefficient mode (BASELINE config 5, `--fp32-smoother`).

With smoother precision 32 the oracle runs exactly the smooth() calls that the HIP plugin runs as sweep pairs on fp32 copies of
Dinv, alpha and beta_i/j/k on copies rounded the same way, (double)(float)v; everything else stays fp64.  The GPU suite pins the
HIP path to this mode bit for bit (tests/test_gpu_fp32_smoother.py).  Here, without a GPU: the mode changes nothing where no
level qualifies or where the smoother, the operator or the boundary condition keeps the levels off the sweep pairs, and where it
does apply it stays inside the tolerance config 5 is documented with."""
import ctypes
import os
import re
import subprocess

import pytest

from hpgmg_testlib import ROOT, VARIANTS, load_golden, split_variant

GOLD = load_golden("fcycle_norms.json")


def fmt(x):
    return "%1.15e" % x


@pytest.fixture
def fp32(oracle):
    """The oracle library with smoother precision 32 for the duration of one test."""
    oracle.lib.hpgmg_fp32_pair_smooths.restype = ctypes.c_longlong
    oracle.lib.hpgmg_set_smoother_precision.argtypes = [ctypes.c_int]
    oracle.lib.hpgmg_set_smoother_precision(32)
    try:
        assert oracle.lib.hpgmg_get_smoother_precision() == 32
        yield oracle
    finally:
        oracle.lib.hpgmg_set_smoother_precision(64)


def solve(be, variant, args):
    """F-cycle norms at h, 2h, 4h, Richardson error and order, and how many smooth() calls ran on rounded coefficients."""
    base, bc = split_variant(variant)
    be.configure(**VARIANTS[base])
    before = be.lib.hpgmg_fp32_pair_smooths()
    s = be.solver_cli(*map(int, args.split()), bc=bc)
    try:
        norms = s.three_sizes()
        err, order = s.richardson()
    finally:
        s.destroy()
    return norms, err, order, be.lib.hpgmg_fp32_pair_smooths() - before


def test_default_precision_is_64(oracle):
    assert oracle.lib.hpgmg_get_smoother_precision() == 64


@pytest.mark.parametrize("variant", ["7pt-cheby-helm", "7pt-cheby", "7ptcc-cheby"])
def test_no_level_qualifies_at_64_cubed(fp32, variant):
    """`5 8`: the fine level has 64^3 cells, below the two million of the sweep-pair threshold -- fp64 lines, no rounded smooth."""
    gold = GOLD[f"{variant} 5 8"]
    norms, err, order, rounded = solve(fp32, variant, "5 8")
    assert rounded == 0
    assert [fmt(v) for v in norms] == gold["norms"]
    assert fmt(err) == gold["richardson_error"] and "%0.3f" % order == gold["order"]


@pytest.mark.parametrize("variant", ["7pt-cheby-helm", "7pt-cheby", "7ptcc-cheby"])
def test_fp32_coefficients_at_256_cubed_stay_inside_the_config5_gate(fp32, variant):
    """`7 8`: the 256^3 and 128^3 levels (>= 2 M cells) smooth on rounded coefficients, the 64^3 level does not.  The h and 2h norms
    move away from the fp64 golden values but stay inside the gate of the GPU test of config 5 (2e-4 relative on the norms, 1e-7
    relative on the Richardson error, the same order); the 4h norm is the golden string itself."""
    gold = GOLD[f"{variant} 7 8"]
    ref = [float(r) for r in gold["norms"]]
    norms, err, order, rounded = solve(fp32, variant, "7 8")
    assert rounded > 0
    for l in (0, 1):
        assert fmt(norms[l]) != gold["norms"][l], (l, norms[l])
        assert abs(norms[l] - ref[l]) <= 2e-4 * ref[l], (l, norms[l], ref[l])
    assert fmt(norms[2]) == gold["norms"][2]
    assert abs(err - float(gold["richardson_error"])) <= 1e-7 * float(gold["richardson_error"]), (err, gold["richardson_error"])
    assert "%0.3f" % order == gold["order"]


def test_the_threshold_follows_hpgmg_set_pair_min_cells(fp32):
    """The same size rule as the HIP plugin's: with the threshold raised above 128^3 cells, `6 8` (fine level 128^3) runs fp64 throughout."""
    fp32.lib.hpgmg_set_pair_min_cells.argtypes = [ctypes.c_longlong]
    gold = GOLD["7pt-cheby-helm 6 8"]
    try:
        fp32.lib.hpgmg_set_pair_min_cells(128 ** 3 + 1)
        norms, _, _, rounded = solve(fp32, "7pt-cheby-helm", "6 8")
        assert rounded == 0 and [fmt(v) for v in norms] == gold["norms"]
        fp32.lib.hpgmg_set_pair_min_cells(0)              # back to the default, 2 000 000
        norms, _, _, rounded = solve(fp32, "7pt-cheby-helm", "6 8")
        assert rounded > 0 and fmt(norms[0]) != gold["norms"][0] and [fmt(v) for v in norms[1:]] == gold["norms"][1:]
    finally:
        fp32.lib.hpgmg_set_pair_min_cells(0)


@pytest.mark.parametrize("variant,args", [("7pt-gsrb", "6 8"), ("27pt-cheby", "6 8"), ("7pt-cheby-periodic", "6 8"), ("7pt-cheby-helm-periodic", "6 8"),
                                          ("7pt-jacobi", "6 8"), ("fv4-cheby", "6 8")])
def test_precision_32_changes_nothing_off_the_sweep_pairs(oracle, fp32, variant, args):
    """Levels big enough for sweep pairs that the smoother, the operator or the boundary condition keeps off them: the fp32 mode leaves
    every number as it is (and where the reference's golden numbers exist, they are those)."""
    got = solve(fp32, variant, args)
    assert got[3] == 0
    fp32.lib.hpgmg_set_smoother_precision(64)
    want = solve(oracle, variant, args)
    assert got == want
    if f"{variant} {args}" in GOLD:
        assert [fmt(v) for v in got[0]] == GOLD[f"{variant} {args}"]["norms"]


PINNED = re.compile(r"f-cycle|\|\|error\|\||order=|eigenvalue")


def cli_lines(args, **env):
    exe = os.path.join(ROOT, "oracle", "hpgmg-fv-oracle")
    out = subprocess.run([exe, "--warmup", "0", "--solves", "1"] + args.split(), capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, OMP_WAIT_POLICY="passive", **env))
    assert out.returncode == 0, (args, out.stdout[-800:], out.stderr[-800:])
    return [re.sub(r"  done \(.*", "", l).strip() for l in out.stdout.splitlines() if PINNED.search(l)]


def test_oracle_executable_takes_the_flag_and_the_environment_variable(fp32):
    """`hpgmg-fv-oracle --fp32-smoother` and HPGMG_SMOOTHER_PRECISION=32 both select the mode (before, the flag was accepted and
    ignored); the f-cycle norms they print are the library's."""
    norms = solve(fp32, "7pt-cheby-helm", "6 8")[0]
    flag = cli_lines("--fp32-smoother --helmholtz 6 8")
    envv = cli_lines("--helmholtz 6 8", HPGMG_SMOOTHER_PRECISION="32")
    plain = cli_lines("--helmholtz 6 8")
    assert len(flag) >= 10 and flag == envv and flag != plain
    printed = [re.search(r"norm=(\S+)", l).group(1) for l in flag if "f-cycle" in l]
    assert [n for n in (fmt(v) for v in norms) if n in printed] == [fmt(v) for v in norms], (norms, printed)
