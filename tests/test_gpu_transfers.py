"""The transfer kernels of kernels/blocks.hip -- restrict_blocks_kernel, restrict_cell_zero_kernel, interp_blocks_kernel, interp_tensor_kernel -- against
the CPU oracle at their launch edges, through the operators that launch them: restriction, hpgmg_restrict_zero_fused, interpolation_vcycle,
interpolation_fcycle and hpgmg_zero_interpolation_fcycle_fused.  The rows, and the edge each exists for, are the tables of tests/transfer_lib.py;
tests/test_oracle_transfers.py shows on the CPU that every row holds its edge, that the oracle is the reference's arithmetic, and that the data can tell
a wrong kernel.  Every comparison is transfer_lib.same_bits (np.array_equal on bits, every NaN the one NaN).

Whole padded boxes -- interior, ghost cells and padding -- are compared wherever the operator defines them: the restrictions (only the cells the lists
name may change: the target is pre-filled with NaN), restriction + zero_vector as one launch (the zeroed vector: interior and ghost cells 0.0, padding
untouched, as zero_vector leaves it), and the two interpolations (fine target, and the coarse operand whose ghost cells the operator fills).  Interiors
are compared for hpgmg_zero_interpolation_fcycle_fused, which leaves the fine ghost cells as scratch (operators_hip.c).

The `prescale == 0` rule ("The `prescale == 0` rule"): the kernels fetch the old fine value only for a result that is a zero, so a NaN or Inf old value survives
only there; where the interpolant is not a zero it is dropped, and the reference's 0 * NaN = NaN does not appear.  test_prescale_zero_on_special_values
holds the kernels to exactly that (transfer_lib.expected_at_prescale_zero) and to the reference everywhere else, the sign of every zero included.

Left out, deliberately:
* The non-temporal instances (NT) need a fine level above 256 MB; they stay with the full-size F-cycle goldens.
* Send-buffer entries (write.box < 0) and increment_blocks exist only across ranks.

The scalar-store path (Lf.flags & 1 == 0) is reachable on an even-sized one-rank level: plugin_runtime.c sets the flag only if jStride, kStride and volume
are even and every box's first interior cell is 16-byte aligned, and hpgmg_set_box_alignment(jstride = an odd number above the padded width) makes create_vectors
(level.c) give every level that odd jStride.  test_the_scalar_store_path runs one trilinear and one fv4 row under it and restores the alignment.  Every kernel
takes such a level: the only 16-byte accesses to a level's vectors are the pairs of blocks.hip, norm_copy_restrict (blas1.hip), the sweep pairs (pair.hip) and
the wide 7-point kernel (stencil.hip), and each of their launchers asks `flags & 1`.

Rows of the 27-point, fv2 and fv4 plugins on box sides that are no power of two -- (1, 12), (1, 24), (1, 40), (1, 72) and (1, 136): no other test runs
these plugins there, and MGBuild rebuilds the operator on every coarse level (sides 6, 3; 12, 6, 3; 20, 10, 5; 36, 18, 9; 68, 34, 17), where a launcher
that refused the level would abort the process.  All three plugins take every one of these levels; from the code:
* rebuild_operator (plugin_problem.c:130-144) issues restrictions, extrapolate_betas, exchange_boundary and rebuild_operator_blackbox.  Restrictions and
  exchanges are block lists (hpgmg_hip_restrict_blocks / _copy_blocks: no predicate on the level); extrapolate_betas_kernel picks its formula by
  `L.dim >= 5 / >= 4 / >= 2`.
* rebuild_operator_blackbox (plugin_ghosts.c:291-317) issues color_vector, exchange_boundary, apply_BCs and hpgmg_hip_blackbox_accumulate / _finalize.
  apply_BCs_p2 / _v2 / _v4 (plugin_ghosts.c:161-281) fall back below sides 2 / 2 / 4 and refuse nothing else (bc_fv_clear_mode of blocks.hip asks order and
  ghost depth only); hpgmg_hip_blackbox_accumulate (stencil.hip:453-457) goes to launch27<MODE_BLACKBOX> / launch_direct<MODE_BLACKBOX>, whose tiled branches
  exclude MODE_BLACKBOX (stencil.hip:87, :184), so the probe always runs stencil27_kernel / stencil_direct_kernel (fv2: the 7-point variant, in
  kDirectVariants) on plan()'s rounded-up tiles -- both kernels return for `i >= L.dim || j >= L.dim` and clamp k (stencil_untiled.hpp:27-28, :77-78).
* The interpolations themselves ask hp_exchange_and_bcs_one_launch (plugin_ghosts.c:41-57: sides >= 2, >= 4 for order 4; else the three-step form), then
  hpgmg_hip_interpolate_blocks, which has no predicate on the level.  MGBuild runs no smoother and no fused residual form.
"""
import numpy as np
import pytest

import hpgmg_amd as H
import transfer_lib as X
from hpgmg_testlib import seeded_field

pytestmark = pytest.mark.gpu

U, F, E, R = H.VECTOR_U, H.VECTOR_F, H.VECTOR_E, H.VECTOR_R


@pytest.fixture(scope="module")
def pairs(hip, oracle):
    held = X.Hierarchies(hip, oracle)
    X.declare_fused(hip.lib)
    yield held
    held.close()


def row_pair(pairs, row):
    hh, ho = X.pair_of(pairs, row.plugin, row.geom)
    X.check_row(row, hh)
    return hh, ho


def on_both(hs, fn):
    out = []
    for h in hs:
        h.configure()
        out.append(fn(h))
    return out


@pytest.mark.parametrize("row", X.RESTRICTION_ROWS, ids=X.row_id)
def test_restrictions(pairs, row):
    """All four types, from a coefficient vector to a plain one, from coefficient to coefficient (what MGBuild does) and from plain to plain (U, its
    ghost copies exchanged first: a coarse face has two writers).  Whole padded coarse boxes, pre-filled with NaN."""
    hs = row_pair(pairs, row)
    on_both(hs, lambda h: h.be.lib.exchange_boundary(h.fine.ptr, U, H.STENCIL_SHAPE_BOX))
    for rtype in X.TYPES:
        for id_c, id_f in ((R, X.SOURCE_OF[rtype]), (X.SOURCE_OF[rtype], X.SOURCE_OF[rtype]), (E, U)):
            def run(h):
                saved = h.coarse.read_all(id_c)
                h.coarse.write_all(id_c, X.nan_field(h.coarse))
                h.be.lib.restriction(h.coarse.ptr, id_c, h.fine.ptr, id_f, rtype)
                got = h.coarse.read_all(id_c)
                h.coarse.write_all(id_c, saved)
                return got
            got, want = on_both(hs, run)
            assert not np.isnan(X.interior_of(hs[1].coarse, want)).any()
            assert X.same_bits(got, want), (rtype, id_c, id_f, X.differing(got, want))


@pytest.mark.parametrize("row", X.RESTRICT_ZERO_ROWS, ids=X.row_id)
def test_restriction_and_zero_vector_as_one_launch(pairs, row):
    """hpgmg_restrict_zero_fused against restriction + zero_vector: the coarse target and the zeroed vector, whole padded boxes, both pre-filled with
    NaN in ghost cells and padding too.  With zero_id == id_c it returns 0 and touches nothing."""
    hh, ho = row_pair(pairs, row)
    for h in (hh, ho):
        for vid in (R, U):
            h.coarse.write_all(vid, X.nan_field(h.coarse))
    hh.configure()
    assert hh.be.lib.hpgmg_restrict_zero_fused(hh.coarse.ptr, R, hh.fine.ptr, F, U) == 1
    ho.configure()
    ho.be.lib.restriction(ho.coarse.ptr, R, ho.fine.ptr, F, H.RESTRICT_CELL)
    ho.be.lib.zero_vector(ho.coarse.ptr, U)
    for vid in (R, U):
        got, want = hh.coarse.read_all(vid), ho.coarse.read_all(vid)
        assert X.same_bits(got, want), (vid, X.differing(got, want))
    assert not X.interior_of(ho.coarse, ho.coarse.read_all(U)).any() and not np.isnan(X.interior_of(ho.coarse, ho.coarse.read_all(R))).any()
    hh.configure()
    hh.coarse.write_all(R, X.nan_field(hh.coarse))
    assert hh.be.lib.hpgmg_restrict_zero_fused(hh.coarse.ptr, R, hh.fine.ptr, F, R) == 0
    assert np.isnan(hh.coarse.read_all(R)).all()


@pytest.mark.parametrize("row", X.INTERPOLATION_ROWS, ids=X.row_id)
def test_interpolations(pairs, row):
    """interpolation_vcycle and interpolation_fcycle at four prescales on random data: the fine target and the coarse operand, whole padded boxes."""
    hs = row_pair(pairs, row)
    for which in ("vcycle", "fcycle"):
        for n, prescale in enumerate(X.PRESCALES):
            old, coarse = seeded_field(hs[0].fine, 40 + n), seeded_field(hs[0].coarse, 50 + n)
            (got, got_c), (want, want_c) = on_both(hs, lambda h: X.run_interpolation(h, which, prescale, old, coarse))
            assert X.same_bits(got, want), (which, prescale, X.differing(got, want))
            assert X.same_bits(got_c, want_c), (which, prescale, "coarse operand", X.differing(got_c, want_c))


SPECIAL = [(row, which) for row in X.SPECIAL_ROWS for which in ("vcycle", "fcycle")]


@pytest.mark.parametrize("row,which", SPECIAL, ids=[f"{X.row_id(r)}-{w}" for r, w in SPECIAL])
def test_prescale_zero_on_special_values(pairs, row, which):
    """Coarse cubes of +0.0 and -0.0 under an old fine field of +0.0, -0.0, positive, negative, NaN and +Inf: the re-read branch, the sign of every zero
    result, and the stated exception -- a non-finite old value is dropped exactly where the interpolant is not a zero."""
    hh, ho = row_pair(pairs, row)
    ho.configure()
    case = X.special_case(ho, which)
    assert case.dropped.any() and (case.clean[~np.isfinite(case.old)] == 0.0).any()
    hh.configure()
    got, _ = X.run_interpolation(hh, which, 0.0, case.old, case.coarse)
    assert X.same_bits(got, case.expected), (X.order_of(hh, which), X.differing(got, case.expected))


@pytest.mark.parametrize("row", X.ZERO_INTERPOLATION_ROWS, ids=X.row_id)
def test_zero_vector_and_interpolation_as_one_launch(pairs, row):
    """hpgmg_zero_interpolation_fcycle_fused (orders 17 ... 20) against zero_vector + interpolation_fcycle, interiors.  The fine vector holds NaN, Inf
    and numbers of size 1e3 beforehand; the zeroed forms never read it, so none of that may show."""
    hh, ho = row_pair(pairs, row)
    coarse = seeded_field(hh.coarse, 61)
    junk = X.old_special(hh.fine)[0] * 1e3
    hh.configure()
    hh.fine.write_all(E, junk)
    hh.coarse.write_all(R, coarse)
    assert hh.be.lib.hpgmg_zero_interpolation_fcycle_fused(hh.fine.ptr, E, hh.coarse.ptr, R) == 1
    ho.configure()
    ho.fine.write_all(E, junk)
    ho.coarse.write_all(R, coarse)
    ho.be.lib.zero_vector(ho.fine.ptr, E)
    ho.be.lib.interpolation_fcycle(ho.fine.ptr, E, 0.0, ho.coarse.ptr, R)
    got, want = X.interior_of(hh.fine, hh.fine.read_all(E)), X.interior_of(ho.fine, ho.fine.read_all(E))
    assert np.isfinite(got).all()
    assert X.same_bits(got, want), X.differing(got, want)


@pytest.mark.parametrize("plugin,geom,jstride", [("7pt", (2, 16), 19), ("fv4", (2, 16), 21)], ids=["7pt-2x16", "fv4-2x16"])
def test_the_scalar_store_path(hip, oracle, plugin, geom, jstride):
    """Levels whose rows are an odd number of doubles apart: `pairs` is false in both interpolation kernels, the children go out as two 8-byte stores and the
    old values come in as two 8-byte loads.  Both interpolations at the four prescales, the special values at prescale 0, and the zeroed form."""
    held = X.Hierarchies(hip, oracle)
    X.declare_fused(hip.lib)
    for be in (hip, oracle):
        be.lib.hpgmg_set_box_alignment(jstride, 0, 0, 0)               # (0: that alignment stays as it is)
    try:
        hh, ho = X.pair_of(held, plugin, geom)
        for lv in (hh.fine, hh.coarse):
            assert lv.jStride == jstride and lv.jStride % 2 == 1        # -> flags & 1 == 0 (plugin_runtime.c: "all strides even")
        for which in ("vcycle", "fcycle"):
            for n, prescale in enumerate(X.PRESCALES):
                old, coarse = seeded_field(hh.fine, 70 + n), seeded_field(hh.coarse, 80 + n)
                (got, got_c), (want, want_c) = on_both((hh, ho), lambda h: X.run_interpolation(h, which, prescale, old, coarse))
                assert X.same_bits(got, want) and X.same_bits(got_c, want_c), (which, prescale, X.differing(got, want))
            ho.configure()
            case = X.special_case(ho, which)
            hh.configure()
            got, _ = X.run_interpolation(hh, which, 0.0, case.old, case.coarse)
            assert case.dropped.any() and X.same_bits(got, case.expected), (which, X.differing(got, case.expected))
        junk, coarse = X.old_special(hh.fine)[0] * 1e3, seeded_field(hh.coarse, 91)
        for h in (hh, ho):
            h.configure()
            h.fine.write_all(E, junk)
            h.coarse.write_all(R, coarse)
        hh.configure()
        assert hh.be.lib.hpgmg_zero_interpolation_fcycle_fused(hh.fine.ptr, E, hh.coarse.ptr, R) == 1
        ho.configure()
        ho.be.lib.zero_vector(ho.fine.ptr, E)
        ho.be.lib.interpolation_fcycle(ho.fine.ptr, E, 0.0, ho.coarse.ptr, R)
        got, want = X.interior_of(hh.fine, hh.fine.read_all(E)), X.interior_of(ho.fine, ho.fine.read_all(E))
        assert np.isfinite(got).all() and X.same_bits(got, want), X.differing(got, want)
    finally:
        held.close()
        for be in (hip, oracle):
            be.lib.hpgmg_set_box_alignment(4, 4, 4, 32)                # the defaults of level.c
