"""BASELINE config 5, the mixed-precision Chebyshev smoother (`--fp32-smoother`, hpgmg_set_smoother_precision(32)), pinned bit for bit.

The sweep-pair kernel with fp32 coefficient streams (cheby_pair.hpp: CoefStream<true>) is the fp64 kernel with only its loads of Dinv, alpha and
beta_i/j/k changed, and (double)(float)v widens exactly.  So it must equal the CPU oracle run on those five vectors rounded elementwise to fp32:
per smooth() (every geometry of the fp64 sweep-pair tests, the interpolation folded in, a change of the coefficients after the fp32 copies were
made), and per executable run against the oracle's own fp32 mode (oracle/operators_cpu.c: fp32_pair_smooth), in every launch shape of the kernel.
Where the smoother, the operator or the boundary condition keeps the levels off the sweep pairs, the flag must change nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, VARIANTS, load_golden, seeded_field
from test_gpu_operators import make_pair, same
from test_gpu_parity_sweep import pinned_lines

pytestmark = pytest.mark.gpu

COEFS = (H.VECTOR_DINV, H.VECTOR_ALPHA, H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
HIP_EXE = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")
ORACLE_EXE = os.path.join(ROOT, "oracle", "hpgmg-fv-oracle")
GOLD = load_golden("fcycle_norms.json")


@pytest.fixture
def precision(hip, oracle):
    """set(bits) switches the HIP plugin's smoother precision; both libraries are back at 64 after the test.  The oracle stays at 64 in the
    operator tests: it is handed rounded coefficients instead (rounding them again would change nothing)."""
    for be in (hip, oracle):
        be.lib.hpgmg_set_smoother_precision.argtypes = [ctypes.c_int]
        be.lib.hpgmg_fp32_pair_smooths.restype = ctypes.c_longlong
        be.lib.hpgmg_set_smoother_precision(64)
    try:
        yield lambda bits: hip.lib.hpgmg_set_smoother_precision(bits)
    finally:
        for be in (hip, oracle):
            be.lib.hpgmg_set_smoother_precision(64)


def ab(variant):
    return (1.0, 1.0) if "helm" in variant else (0.0, 1.0)


def rounded(x):
    return x.astype(np.float32).astype(np.float64)


def coefficients(lv):
    """The five coefficient vectors of a level, whole padded boxes (the kernels read the ghost faces of the betas)."""
    return {vid: lv.read_all(vid) for vid in COEFS if vid < lv.num_vectors}


def write_coefficients(lv, coefs):
    for vid, c in coefs.items():
        lv.write_all(vid, c)


def interiors(lv, vid):
    g, d, w = lv.ghosts, lv.box_dim, lv.box_dim + 2 * lv.ghosts
    a = lv.read_all(vid)
    return a[:, : w * lv.kStride].reshape(-1, w, lv.kStride)[:, :, : w * lv.jStride].reshape(-1, w, w, lv.jStride)[:, g:g + d, g:g + d, g:g + d]


def start_from(levels, state):
    for lv in levels:
        for vid, v in state.items():
            lv.write_all(vid, v)


# the geometries of test_fused_chebyshev_sweep_pairs: one and three 128-cell i tiles, two, boxes of 64 and 32 cells (rows of 128 spanning 2 / 4 boxes)
PAIR_CASES = [("7pt-cheby-helm", (2, 128)), ("7pt-cheby", (1, 128)), ("7ptcc-cheby", (1, 256)), ("7pt-cheby-helm", (3, 128)),
              ("7pt-cheby-helm", (4, 64)), ("7pt-cheby", (8, 32)), ("7pt-cheby", (2, 128)), ("7ptcc-cheby", (4, 64))]


@pytest.mark.parametrize("variant,geom", PAIR_CASES)
def test_fp32_sweep_pairs_equal_the_oracle_on_rounded_coefficients(hip, oracle, precision, variant, geom):
    """smooth() with precision 32: U and VECTOR_TEMP equal the oracle's four fp64 sweeps on the five coefficient vectors rounded to fp32,
    bit for bit over the interiors; and differ from the oracle on the unrounded ones (the fp32 streams were read)."""
    lh, lo = make_pair(hip, oracle, variant, *geom, seed=11)
    try:
        a, b = ab(variant)
        for lv in (lh, lo):
            lv.b.lib.rebuild_operator(lv.ptr, None, a, b)
        assert lh.eigenvalue == lo.eigenvalue
        state = {H.VECTOR_U: lh.read_all(H.VECTOR_U), H.VECTOR_TEMP: lh.read_all(H.VECTOR_TEMP)}
        start_from([lo], state)
        lo.b.lib.smooth(lo.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
        fp64 = interiors(lo, H.VECTOR_U)
        write_coefficients(lo, {vid: rounded(c) for vid, c in coefficients(lh).items()})
        start_from([lh, lo], state)
        precision(32)
        before = hip.lib.hpgmg_fp32_pair_smooths()
        for lv in (lh, lo):
            lv.b.lib.smooth(lv.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
        assert hip.lib.hpgmg_fp32_pair_smooths() == before + 1
        same(lh, lo, [H.VECTOR_U, H.VECTOR_TEMP], interior_only=True)
        assert not np.array_equal(interiors(lh, H.VECTOR_U), fp64)
    finally:
        lh.destroy(); lo.destroy()


@pytest.mark.parametrize("variant,geom", [("7pt-cheby-helm", (2, 128)), ("7ptcc-cheby", (1, 256)), ("7pt-cheby-helm", (2, 64)), ("7pt-cheby", (4, 32))])
def test_fp32_interpolation_folded_into_the_first_sweep_pair(hip, oracle, precision, variant, geom):
    """hpgmg_interp_smooth_fused with precision 32 (the up-leg of MGVCycle on a sweep-pair level of config 5) equals the oracle's
    interpolation_vcycle + smooth() on rounded coefficients bit for bit, and differs from them on the unrounded ones."""
    from hpgmg_testlib import Level
    pairs = []
    for be in (hip, oracle):
        be.configure(**VARIANTS[variant])
        fine = be.level(*geom)
        for vid in range(fine.num_vectors):
            d = seeded_field(fine, 1700 + vid)
            if vid >= H.VECTOR_DINV:
                d = np.abs(d) + 0.5
            fine.write_all(vid, d)
        for vid in range(H.VECTOR_DINV, fine.num_vectors):
            be.lib.exchange_boundary(fine.ptr, vid, H.STENCIL_SHAPE_BOX)
        a, b = ab(variant)
        mg = be.lib.hpgmg_mg_create(fine.ptr, a, b, 1)
        be.lib.rebuild_operator(fine.ptr, None, a, b)
        pairs.append((be, fine, mg))
    try:
        (bh, fh, mh), (bo, fo, mo) = pairs
        a, b = ab(variant)
        hip.lib.hpgmg_interp_smooth_fused.restype = ctypes.c_int
        hip.lib.hpgmg_interp_smooth_fused.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
        ch, co = Level(bh, bh.lib.hpgmg_mg_level(mh, 1)), Level(bo, bo.lib.hpgmg_mg_level(mo, 1))
        coarse_e = seeded_field(ch, 1777)
        ch.write_all(H.VECTOR_U, coarse_e); co.write_all(H.VECTOR_U, coarse_e)
        state = {H.VECTOR_U: fh.read_all(H.VECTOR_U), H.VECTOR_TEMP: fh.read_all(H.VECTOR_TEMP)}
        start_from([fo], state)
        bo.lib.interpolation_vcycle(fo.ptr, H.VECTOR_U, 1.0, co.ptr, H.VECTOR_U)
        bo.lib.smooth(fo.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
        fp64 = interiors(fo, H.VECTOR_U)
        write_coefficients(fo, {vid: rounded(c) for vid, c in coefficients(fh).items()})
        start_from([fh, fo], state)
        precision(32)
        before = hip.lib.hpgmg_fp32_pair_smooths()
        assert hip.lib.hpgmg_interp_smooth_fused(fh.ptr, H.VECTOR_U, H.VECTOR_F, ch.ptr, a, b) == 1
        assert hip.lib.hpgmg_fp32_pair_smooths() == before + 1
        bo.lib.interpolation_vcycle(fo.ptr, H.VECTOR_U, 1.0, co.ptr, H.VECTOR_U)
        bo.lib.smooth(fo.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
        same(fh, fo, [H.VECTOR_U], interior_only=True)      # VECTOR_TEMP is scratch to this cycle-only hook
        assert not np.array_equal(interiors(fh, H.VECTOR_U), fp64)
    finally:
        for be, f, m in pairs:
            be.lib.hpgmg_mg_destroy(m); f.destroy()


@pytest.mark.parametrize("variant,geom", [("7pt-cheby-helm", (2, 128)), ("7pt-cheby", (4, 64))])      # two i tiles: the fp64 pre-pass reads packed coefficients
def test_fp32_copies_and_packed_coefficients_follow_a_rebuild(hip, oracle, precision, variant, geom):
    """One level smoothed in turn with precision 64 and 32, then given new coefficients (betas, alpha) and rebuilt, then smoothed with 32, 64 and
    32 again.  Each smooth() equals the oracle -- on rounded coefficients with 32, on its own with 64 -- from the same starting state: neither the
    fp32 copies nor the packed coefficients of the fp64 pre-pass may outlive the rebuild."""
    lh, lo = make_pair(hip, oracle, variant, *geom, seed=13)
    a, b = ab(variant)
    try:
        def rebuild():
            for lv in (lh, lo):
                lv.b.lib.rebuild_operator(lv.ptr, None, a, b)
            assert lh.eigenvalue == lo.eigenvalue
            return coefficients(lo)

        state = {H.VECTOR_U: lh.read_all(H.VECTOR_U), H.VECTOR_TEMP: lh.read_all(H.VECTOR_TEMP)}

        def step(bits, own):
            precision(bits)
            write_coefficients(lo, {vid: rounded(c) for vid, c in coefficients(lh).items()} if bits == 32 else own)
            start_from([lh, lo], state)
            before = hip.lib.hpgmg_fp32_pair_smooths()
            for lv in (lh, lo):
                lv.b.lib.smooth(lv.ptr, H.VECTOR_U, H.VECTOR_F, a, b)
            assert hip.lib.hpgmg_fp32_pair_smooths() == before + (1 if bits == 32 else 0)
            same(lh, lo, [H.VECTOR_U, H.VECTOR_TEMP], interior_only=True)
            return interiors(lh, H.VECTOR_U)

        own = rebuild()
        old64 = step(64, own)           # packs the pre-pass coefficients
        old32 = step(32, own)           # makes the fp32 copies
        assert not np.array_equal(old64, old32)
        for vid in (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K, H.VECTOR_ALPHA):
            if vid < lh.num_vectors:
                d = np.abs(seeded_field(lh, 1300 + vid)) + 0.25
                lh.write_all(vid, d); lo.write_all(vid, d)
        own = rebuild()
        new32 = step(32, own)
        assert not np.array_equal(new32, old32)
        new64 = step(64, own)
        assert not np.array_equal(new64, old64) and not np.array_equal(new64, new32)
        assert np.array_equal(step(32, own), new32)
    finally:
        lh.destroy(); lo.destroy()


_ORACLE_LINES = {}


def oracle_fp32_lines(flags, size):
    if (flags, size) not in _ORACLE_LINES:
        _ORACLE_LINES[(flags, size)] = pinned_lines(ORACLE_EXE, "--fp32-smoother " + flags, size)
    return _ORACLE_LINES[(flags, size)]


def first_difference(x, y):
    return [p for p in zip(x, y) if p[0] != p[1]][:3]


def fcycle_norms(lines):
    return [re.search(r"norm=(\S+)", l).group(1) for l in lines if "f-cycle" in l]


@pytest.mark.parametrize("flags,size,variant", [("--helmholtz", "7 8", "7pt-cheby-helm"), ("", "7 8", "7pt-cheby"), ("--const-coeff", "7 8", "7ptcc-cheby"),
                                                ("--helmholtz", "6 8", "7pt-cheby-helm"), ("--helmholtz", "8 8", None)])
def test_fp32_smoother_executable_prints_the_oracle_lines(flags, size, variant):
    """`hpgmg-fv --fp32-smoother` and `hpgmg-fv-oracle --fp32-smoother` print the same pinned lines (f-cycle norms at h / 2h / 4h, eigenvalue
    bounds, Richardson error and order).  Fine levels of 128^3 (boxes of 64), 256^3 and 512^3; the fine level's norm is not the fp64 one."""
    hip = pinned_lines(HIP_EXE, "--fp32-smoother " + flags, size)
    cpu = oracle_fp32_lines(flags, size)
    assert len(hip) >= 10 and hip == cpu, first_difference(hip, cpu)
    if variant:
        assert GOLD[f"{variant} {size}"]["norms"][0] not in fcycle_norms(hip)


@pytest.mark.parametrize("flags,size,nw,kc", [("--helmholtz", "7 8", 10, 0), ("--helmholtz", "7 8", 12, 0), ("--helmholtz", "7 8", 16, 0),
                                              ("--helmholtz", "7 8", 10, 24), ("--helmholtz", "7 8", 12, 13), ("--helmholtz", "6 8", 16, 48)])
def test_every_launch_shape_of_the_fp32_sweep_pairs_prints_the_oracle_lines(flags, size, nw, kc):
    """The fp32 instances of the sweep-pair kernel in every shape, forced through HPGMG_TUNE_PAIR_NW / HPGMG_TUNE_PAIR_KC -- the 10-wave ones,
    which the cost model never picks with fp32 streams, and k chunks that leave the last chunk of a level partial (24 and 13 of 256 and 128
    planes, 48 of 128) -- print the oracle's fp32 lines."""
    hip = pinned_lines(HIP_EXE, "--fp32-smoother " + flags, size, HPGMG_TUNE_PAIR_NW=str(nw), HPGMG_TUNE_PAIR_KC=str(kc))
    cpu = oracle_fp32_lines(flags, size)
    assert len(hip) >= 10 and hip == cpu, first_difference(hip, cpu)


@pytest.mark.parametrize("flags,size,golden", [("--smoother gsrb", "7 8", "7pt-gsrb 7 8"), ("--op 27pt", "6 8", "27pt-cheby 6 8"), ("--periodic", "6 8", None)])
def test_fp32_smoother_flag_changes_nothing_off_the_sweep_pairs(flags, size, golden):
    """Levels big enough for sweep pairs that the smoother (GSRB), the operator (27-point) or the boundary condition (periodic) keeps off the
    fp32 path: the flag leaves every line as it is, and those lines hold the reference's golden norms where they exist."""
    plain = pinned_lines(HIP_EXE, flags, size)
    fp32 = pinned_lines(HIP_EXE, "--fp32-smoother " + flags, size)
    assert len(plain) >= 10 and fp32 == plain, first_difference(fp32, plain)
    if golden:
        gold = GOLD[golden]["norms"]
        assert [g for g in gold if g in fcycle_norms(plain)] == gold, (gold, fcycle_norms(plain)[:6])
