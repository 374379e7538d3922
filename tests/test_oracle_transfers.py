"""The transfer operators (restriction, interpolation_vcycle, interpolation_fcycle) on the CPU oracle, at the rows of tests/transfer_lib.py -- the rows
tests/test_gpu_transfers.py then holds kernels/blocks.hip to.

* Every row's edge holds: its predicate over the launch facts read off the level's block lists (transfer_lib.check_row).
* At every 7-point row the oracle's four restrictions, its piecewise-constant and its trilinear interpolation equal the NumPy restatement of the
  reference's summation order bit for bit over WHOLE padded boxes: the target is pre-filled with NaN outside what the operator reads, and only the
  cells the lists name may change.  (The tensor rules p2 / v2 / v4 are not restated: the oracle is their reference, and test_oracle_vs_reference.py
  holds the oracle to the reference's binaries.)
* The data can tell a wrong kernel: three wrong restatements -- the cell sum as a tree of pairs, the trilinear terms with the i and k neighbours in
  each other's place, face I averaged over the J pair alone -- give other bits on the rows that target them, and the same bits on a one-box row where the
  mistake cannot show.
* The special-value fields of the `prescale == 0` rule do what the GPU test assumes: on the oracle alone, for every order 0 ... 4, every reachable
  class (sign of a zero result) x (kind of old value) occurs, and a non-zero interpolant over each non-finite kind of old value.
"""
import numpy as np
import pytest

import hpgmg_amd as H
import hpgmg_testlib as T
import transfer_lib as X

U, F, E, R = H.VECTOR_U, H.VECTOR_F, H.VECTOR_E, H.VECTOR_R


@pytest.fixture(scope="module")
def hierarchy_of():
    """hierarchy_of(plugin, geom): the oracle's hierarchy of a row, kept while the tests stay on that row."""
    held = X.Hierarchies(T.Backend.oracle())
    yield lambda plugin, geom: held.get(plugin, geom)[0]
    held.close()


ALL_ROWS = [(name, row) for name, rows in X.TABLES.items() for row in rows] + [("ragged", row) for row in X.RAGGED_ROWS]
ALL_ROWS.sort(key=lambda nr: (nr[1].plugin, nr[1].geom))


@pytest.mark.parametrize("name,row", ALL_ROWS, ids=[f"{n}-{X.row_id(r)}" for n, r in ALL_ROWS])
def test_every_row_holds_its_edge(hierarchy_of, name, row):
    X.check_row(row, hierarchy_of(row.plugin, row.geom))


SEVEN_POINT_RESTRICTION = [r for r in X.RESTRICTION_ROWS if r.plugin == "7pt"]
SEVEN_POINT_INTERPOLATION = [r for r in X.INTERPOLATION_ROWS if r.plugin == "7pt"]


def restrict_both(h, rtype, id_c, id_f, wrong=None):
    """(the oracle's coarse field, the restatement's), both onto NaN; the fine field is what the level holds.  The coarse vector gets its content back."""
    saved = h.coarse.read_all(id_c)
    h.coarse.write_all(id_c, X.nan_field(h.coarse))
    fine = h.fine.read_all(id_f)
    h.be.lib.restriction(h.coarse.ptr, id_c, h.fine.ptr, id_f, rtype)
    got = h.coarse.read_all(id_c)
    h.coarse.write_all(id_c, saved)
    return got, X.restrict_np(rtype, X.restriction_entries(h, rtype), h.fine, fine, h.coarse, X.nan_field(h.coarse), wrong=wrong)


@pytest.mark.parametrize("row", SEVEN_POINT_RESTRICTION, ids=X.row_id)
def test_restrictions_equal_the_restatement(hierarchy_of, row):
    h = hierarchy_of(row.plugin, row.geom)
    for rtype in X.TYPES:
        for id_c, id_f in ((R, X.SOURCE_OF[rtype]), (X.SOURCE_OF[rtype], X.SOURCE_OF[rtype])):
            got, want = restrict_both(h, rtype, id_c, id_f)
            assert X.same_bits(got, want), (rtype, id_c, X.differing(got, want))
            assert not np.isnan(X.interior_of(h.coarse, got)).any()              # the lists cover every coarse cell


def interpolation_fields(h, prescale, seed):
    """Old fine field (NaN in ghost cells and padding, which no entry names) and coarse field."""
    old = X.nan_field(h.fine)
    X.interior_of(h.fine, old)[...] = X.interior_of(h.fine, T.seeded_field(h.fine, seed))
    return old, T.seeded_field(h.coarse, seed + 1)


@pytest.mark.parametrize("row", SEVEN_POINT_INTERPOLATION, ids=X.row_id)
def test_interpolations_equal_the_restatement(hierarchy_of, row):
    h = hierarchy_of(row.plugin, row.geom)
    lists = X.interpolation_entries(h)
    for which in ("vcycle", "fcycle"):
        for n, prescale in enumerate(X.PRESCALES):
            old, coarse = interpolation_fields(h, prescale, 40 + n)
            got, filled = X.run_interpolation(h, which, prescale, old, coarse)
            want = X.interpolate_np(X.order_of(h, which), lists, h.fine, old, prescale, h.coarse, filled)
            assert X.same_bits(got, want), (which, prescale, X.differing(got, want))
            assert not np.isnan(X.interior_of(h.fine, got)).any()


def control_fields(h):
    """Fields on which none of the three mistakes can show: small integers that depend on j alone, so every sum is exact in any order and the pairs
    along i, j and k hold the same numbers."""
    fine = np.zeros((h.fine.num_boxes, h.fine.volume))
    v = X.box_views(h.fine, fine)
    v[...] = (3.0 + np.arange(v.shape[2]))[None, None, :, None]
    return fine


@pytest.mark.parametrize("wrong,rtype", [("cell-order", H.RESTRICT_CELL), ("face-pairs", H.RESTRICT_FACE_I)])
def test_the_data_can_tell_a_wrong_restriction(hierarchy_of, wrong, rtype):
    for row in SEVEN_POINT_RESTRICTION:
        if row.geom == (1, 2):
            continue                                                             # (one coarse cell: two orders of one sum may agree)
        h = hierarchy_of(row.plugin, row.geom)
        got, other = restrict_both(h, rtype, R, X.SOURCE_OF[rtype], wrong=wrong)
        cells = np.isfinite(got)
        assert np.abs(other[cells] - got[cells]).max() <= (1e-15 if wrong == "cell-order" else 2.0)      # the same sum in another order / another average
        assert not X.same_bits(got, other), (wrong, row.geom)
    h = hierarchy_of("7pt", (1, 2))
    h.fine.write_all(U, control_fields(h))
    got, other = restrict_both(h, rtype, R, U, wrong=wrong)
    assert X.same_bits(got, other) and np.isfinite(got).sum() >= 1


def test_the_data_can_tell_a_wrong_trilinear_order(hierarchy_of):
    """The i and k neighbours carry the same weights, so swapping their roles is the same sum in another order: last bits.  With one coarse cell the
    boundary condition makes the two neighbours the same number, and the mistake cannot show."""
    for row in SEVEN_POINT_INTERPOLATION:
        h = hierarchy_of(row.plugin, row.geom)
        old, coarse = interpolation_fields(h, 0.3, 60)
        got, filled = X.run_interpolation(h, "fcycle", 0.3, old, coarse)
        other = X.interpolate_np(1, X.interpolation_entries(h), h.fine, old, 0.3, h.coarse, filled, wrong="swap-ik")
        cells = np.isfinite(got)
        assert np.abs(other[cells] - got[cells]).max() <= 1e-15
        assert X.same_bits(got, other) == (row.geom == (1, 2)), row.geom


SPECIAL = [(row, which) for row in X.SPECIAL_ROWS for which in ("vcycle", "fcycle")]


@pytest.mark.parametrize("row,which", SPECIAL, ids=[f"{X.row_id(r)}-{w}" for r, w in SPECIAL])
def test_the_special_value_fields_reach_every_class(hierarchy_of, row, which):
    h = hierarchy_of(row.plugin, row.geom)
    order = X.order_of(h, which)
    case = X.special_case(h, which)
    from reduction_lib import cell_offsets
    counts = X.class_counts(case.exact, case.clean, case.kind, cell_offsets(h.fine))
    missing = [c for c in X.reachable_classes(order) if counts[c] < 1]
    assert not missing, (order, missing, counts)
    # a zero result never sits over a non-finite old value, and a -0.0 result only where the arithmetic allows it
    unreachable = [c for c in counts if c[0] in ("+0", "-0", "nan") and c not in X.reachable_classes(order) and counts[c]]
    assert not unreachable, (order, unreachable)
    # the exception is exercised: non-zero interpolants over NaN and over +Inf, where `expected` is the clean value and `exact` is NaN
    q = cell_offsets(h.fine)
    dropped = case.dropped[:, q]
    assert counts["value", "nan"] >= 1 and counts["value", "inf"] >= 1 and dropped.sum() == counts["value", "nan"] + counts["value", "inf"]
    assert np.isnan(case.exact[:, q][dropped]).all() and np.isfinite(case.expected[:, q][dropped]).all()
    assert not case.dropped.any() or not X.same_bits(case.exact, case.expected)


def test_orders_zero_to_four_are_all_covered():
    orders = {X.PLUGINS[row.plugin][k] for row in X.SPECIAL_ROWS for k in (2, 3)}
    assert orders == {0, 1, 2, 3, 4}
    for order in orders:
        geoms = {row.geom[0] * row.geom[1] for row in X.SPECIAL_ROWS if order in X.PLUGINS[row.plugin][2:]}
        assert min(geoms) < 64 <= max(geoms)
