"""The NumPy restatements of tests/reduction_lib.py pinned on the CPU oracle, before tests/test_gpu_reductions.py trusts them: dot, mean and norm of
the oracle (oracle/operators_cpu.c, the order of the reference's misc.c:261-269) equal tile_sum / abs_max bit for bit at every geometry of the GPU
test's tables up to a box side of 136 -- among them the tiles that are no whole 8 x 8 rows (sides 4, 6, 12, 104, 136) --, and the nine element-wise
passes equal their one-line NumPy expressions over whole padded boxes.  The levels have only the vectors a case uses (one, two or ten), far fewer
than an operator reserves: hpgmg_level_create and the BLAS-1 calls take that.  Every build has -ffp-contract=off: nothing here has a tolerance.
"""
import numpy as np
import pytest

import reduction_lib as R
from hpgmg_testlib import VARIANTS

# (boxes per side, box side): the union of the norm and sum tables of test_gpu_reductions.py up to side 136
GEOMS = [(1, 1), (1, 6), (3, 4), (1, 16), (2, 8), (3, 12), (5, 6), (1, 64), (2, 64), (4, 64), (1, 104), (1, 136), (17, 2)]
SUM_GEOMS = [g for g in GEOMS if g not in ((4, 64), (17, 2))]      # (the restatement's Python loop over 4913 boxes proves nothing a smaller one does not)


def _id(g):
    return f"{g[0]}x{g[1]}"


@pytest.fixture(autouse=True)
def _configured(oracle):
    oracle.configure(**VARIANTS["7pt-cheby-helm"])      # one ghost cell; the BLAS-1 operators themselves do not depend on the operator


@pytest.mark.parametrize("geom", SUM_GEOMS, ids=_id)
def test_dot_and_mean_are_the_tile_chains(oracle, geom):
    lv = oracle.level(*geom, num_vectors=2)
    try:
        assert lv.num_vectors == 2 and lv.num_boxes == geom[0] ** 3 and lv.box_dim == geom[1]
        assert not lv.read_raw(0, 1).any()                                          # a created level is zero-filled
        a, b = R.random_field(lv, 11 + geom[1]), R.random_field(lv, 12 + geom[1])
        lv.write_all(0, a); lv.write_all(1, b)
        plan = R.sum_plan(*geom)
        assert len(R.tile_partials(lv, a)) == plan.ntiles
        L = oracle.lib
        assert L.dot(lv.ptr, 0, 1) == R.tile_sum(lv, a, b)
        assert L.dot(lv.ptr, 0, 0) == R.tile_sum(lv, a, a)
        assert L.mean(lv.ptr, 0) == R.mean_of(lv, R.tile_sum(lv, a))
        assert L.norm(lv.ptr, 1) == R.abs_max(lv, b)
    finally:
        lv.destroy()


@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_norm_is_the_largest_interior_magnitude(oracle, geom):
    """One vector; the maximum planted in a ghost-free corner cell, with a larger value in the ghost cell next to it that no norm may see."""
    lv = oracle.level(*geom, num_vectors=1)
    try:
        a = R.random_field(lv, 21 + geom[1])
        q = R.cell_offsets(lv)
        box = lv.num_boxes - 1
        a[box, q[-1, -1, -1]] = -R.HUGE
        a[box, q[-1, -1, -1] + 1] = 7.0 * R.HUGE                                    # the ghost cell past the last interior cell
        lv.write_all(0, a)
        assert oracle.lib.norm(lv.ptr, 0) == R.abs_max(lv, a) == R.HUGE
        if geom != (1, 1):                                                          # (a level of one cell has no second cell)
            a[0, q[0, 0, 0]] = np.nan                                               # a NaN never becomes the norm
            lv.write_raw(0, 0, a[0])
            assert oracle.lib.norm(lv.ptr, 0) == R.abs_max(lv, a, nan=True) == R.HUGE
    finally:
        lv.destroy()


def test_a_chain_in_another_order_is_another_number(oracle):
    """The comparison above has teeth: the same cells chained with j and k swapped, or the tiles chained backwards, give other bits."""
    lv = oracle.level(3, 12, num_vectors=1)
    try:
        a = R.random_field(lv, 5)
        lv.write_all(0, a)
        want = oracle.lib.mean(lv.ptr, 0)

        def swapped(level, x, y=None):
            v, d = R.interior(level, x), level.box_dim
            return np.array([R.chain(v[box, k0:k0 + 8, j0:j0 + 8, :].transpose(1, 0, 2))
                             for box in range(level.num_boxes) for k0 in range(0, d, 8) for j0 in range(0, d, 8)])

        assert R.mean_of(lv, R.tile_sum(lv, a)) == want
        assert R.mean_of(lv, R.tile_sum(lv, a, partials=swapped)) != want
        assert R.mean_of(lv, R.chain(R.tile_partials(lv, a)[::-1])) != want
        assert R.mean_of(lv, R.interior(lv, a).sum()) != want                       # (np.sum is pairwise)
    finally:
        lv.destroy()


@pytest.mark.parametrize("geom", [(1, 72), (1, 3), (1, 1), (3, 12)], ids=_id)
def test_elementwise_passes_are_their_numpy_expressions(oracle, geom):
    lv = oracle.level(*geom, num_vectors=R.EW_VECTORS)
    try:
        assert lv.box_dim == geom[1] and lv.num_vectors == R.EW_VECTORS
        init = R.elementwise_fields(lv, 40 + geom[1])
        for v, x in enumerate(init):
            lv.write_all(v, x)
        R.elementwise_calls(lv)
        for v, want in enumerate(R.elementwise_expected(lv, init)):
            bad = np.argwhere(R.bits(lv.read_all(v)) != R.bits(want))
            assert bad.size == 0, f"vector {v} at (box, raw offset) {bad[:5].tolist()}"
    finally:
        lv.destroy()


def test_launch_arithmetic_tables():
    """The plans the GPU test's docstring tabulates (kernels/blas1.hip: hpgmg_hip_norm_max, ordered_sum; kernels/reduce.hip: final_max_kernel)."""
    n = {g: R.norm_plan(*g) for g in GEOMS}
    assert [(n[g].path, n[g].nblk) for g in ((1, 1), (1, 6), (1, 16))] == [("absmax_small", 1), ("absmax_small", 9), ("absmax_small", 64)]
    assert (n[2, 8].per_box, n[2, 8].partials, n[2, 8].rows_in_flight, n[2, 8].row0_trips) == (16, 128, 1, 1)
    assert (n[3, 12].per_box, n[3, 12].partials, n[3, 12].divide) == (36, 972, True) and R.final_max_plan(972) == (204, 1, 156)
    assert (n[1, 104].per_box, n[1, 104].halvings, n[1, 104].rows_in_flight, n[1, 104].lane_trips) == (2704, 0, 1, 2)
    assert (n[1, 136].per_box, n[1, 136].halvings, n[1, 136].rows_in_flight, n[1, 136].lane_trips) == (2312, 1, 2, 3)
    assert (n[2, 64].per_box, n[2, 64].halvings, n[2, 64].partials, n[2, 64].rows_in_flight) == (512, 1, 4096, 2)
    assert (n[4, 64].per_box, n[4, 64].halvings, n[4, 64].rows_in_flight, n[4, 64].row0_trips) == (64, 4, 4, 4)
    assert (n[17, 2].per_box, n[17, 2].partials) == (1, 4913) and R.final_max_plan(4913) == (256, 5, 4913 - 4 * (5 * 49 + 4 * 207))
    assert R.final_max_plan(512) == (0, 0, 512) and R.final_max_plan(1331) == (256, 1, 307) and R.final_max_plan(8192)[1:] == (8, 0)
    s = {g: R.sum_plan(*g) for g in [(1, 6), (3, 4), (1, 64), (3, 12), (5, 6), (1, 104), (1, 136), (1, 264), (1, 512), (1, 520)]}
    assert [(s[g].ntiles, s[g].kernel) for g in s] == [(1, "tile_sum<true>"), (27, "tile_sum<true>"), (64, "tile_sum<true>"), (108, "wave<2>"), (125, "wave<2>"),
                                                       (169, "wave<2>"), (289, "wave<4>"), (1089, "wave<8>"), (4096, "wave<8>"), (4225, "tile_sum<false>")]
    assert s[3, 12].tile_rows == [64, 32, 16] and s[5, 6].tile_rows == [36] and s[5, 6].groups == [5]
    assert (s[1, 104].live_chunks, s[1, 104].last_chunk_lanes, s[1, 104].tail) == (2, 40, 41)
    assert (s[1, 136].live_chunks, s[1, 136].last_chunk_lanes) == (3, 8) and (s[1, 264].live_chunks, s[1, 264].last_chunk_lanes) == (5, 8)
    assert s[1, 512].lds_bytes == 65536 and s[1, 264].lds_bytes == 33792
