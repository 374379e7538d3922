"""The three block hooks of include/hpgmg_operators.h (hpgmg_block_gram / _combine / _residual) on the CPU oracle, on plain levels:
the portable forms of host/hooks_host.inc must equal the NumPy restatements of tests/block_lib.py as 64-bit patterns, at the rows of pcg_lib.TABLE
that exercise the mapping and at list sizes on the edges of the 6 x 6 pair tile (1, 5, 6, 7, 13, 36) -- the rows and sizes tests/test_gpu_block_hooks.py
then holds kernels/block.hip to.  Every ghost and padding double of every input is NaN and every output is pre-filled with NaN: the results must be
finite and the outputs' ghost and padding doubles keep their bits.  Every unweighted Gram entry is also hpgmg_pcg_dot on its pair, bit for bit.
"""
import numpy as np
import pytest

import block_lib as B
import hpgmg_testlib as T
import pcg_lib as P
from reduction_lib import HUGE, bits, cell_offsets

_kept = {}


@pytest.fixture(scope="module")
def bench_of():
    """bench_of(geom): (level, fields) of one row on the oracle, made once for the module; the level holds the fields."""
    be = T.Backend.oracle()
    be.configure(**T.VARIANTS["7pt-cheby-helm"])

    def get(geom):
        if geom not in _kept:
            P.check_row(geom)
            lv = B.new_level(be, geom)
            F = B.fields_of(lv, 900 + 13 * geom[0] + geom[1])
            B.write_fields(lv, F)
            _kept[geom] = (lv, F)
        return _kept[geom]
    yield get
    while _kept:
        _kept.popitem()[1][0].destroy()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_gram_equals_the_restatement_and_pcg_dot(bench_of, geom, weighted):
    lv, F = bench_of(geom)
    w = B.W_ID if weighted else -1
    for name, (a, b) in B.gram_cases(geom).items():
        rc, G = B.call_gram(lv, a, b, w)
        assert rc == 0 and np.isfinite(G).all(), name
        B.same_bits(G, B.gram_restated(lv, F, a, b, w), f"{B.row_id(geom)} {name}")
        if a == b:
            assert np.array_equal(bits(G), bits(G.T)), name                 # the lower triangle is a copy of the upper
        if not weighted:                                                    # every entry is hpgmg_pcg_dot on its pair (4913 boxes: every fifth entry)
            pairs = [(i, j) for i in range(len(a)) for j in range(len(b))]
            for i, j in pairs[::5] if geom == (17, 4) else pairs:
                took, value = P.call_dot(lv, a[i], b[j])
                assert took == 0 and P.same_scalar(G[i, j], value), (name, i, j)
    assert B.call_gram(lv, a, b, w, host=True)[0] == 0


def test_gram_association_of_the_weight_shows(bench_of):
    """(w * a) * b is not w * (a * b) in floating point: some entry of a weighted request has other bits under the other association, so the
    restatement can tell the two."""
    lv, F = bench_of((1, 12))
    a, b = B.gram_cases((1, 12))["identical-13"]
    q = cell_offsets(lv)
    other = np.array([[P.header_order_dot(F[B.W_ID][:, q], F[va][:, q] * F[vb][:, q], lv.box_dim) for vb in b] for va in a])
    G = B.call_gram(lv, a, b, B.W_ID)[1]
    assert np.allclose(G, other, rtol=0, atol=1e-12) and (bits(np.triu(G)) != bits(np.triu(other))).any()


@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_combine_equals_the_restatement(bench_of, geom):
    lv, F = bench_of(geom)
    nan = np.full((lv.num_boxes, lv.volume), np.nan)
    for n, (name, (out_ids, in_ids, zero)) in enumerate(B.combine_cases(geom).items()):
        C = B.combine_matrix(len(in_ids), len(out_ids), zero, 40 + n)
        held = dict(F)
        for v in out_ids:
            if v not in in_ids:                                             # an output that is no input: every double NaN before the call
                held[v] = nan
        B.write_fields(lv, held, out_ids)
        try:
            assert B.call_combine(lv, out_ids, in_ids, C) == 0, name
            want = B.combine_restated(lv, held, out_ids, in_ids, C)
            q = cell_offsets(lv)
            for j, v in enumerate(out_ids):
                got = lv.read_all(v)
                assert np.isfinite(got[:, q]).all(), (name, v)
                B.same_bits(got, want[v], f"{B.row_id(geom)} {name} output {v}")
                if zero == j:
                    assert (got[:, q] == 0.0).all() and not np.signbit(got[:, q]).any()
            for v in in_ids:
                if v not in out_ids:
                    B.same_bits(lv.read_all(v), F[v], f"{name} input {v}")
        finally:
            B.write_fields(lv, F, out_ids)


def test_combine_refuses_repeated_outputs(bench_of):
    lv, F = bench_of((1, 12))
    nan = np.full((lv.num_boxes, lv.volume), np.nan)
    out_ids, in_ids = [40, 41, 40], [1, 2, 3, 4]
    B.write_fields(lv, {40: nan, 41: nan})
    try:
        for host in (False, True):
            assert B.call_combine(lv, out_ids, in_ids, np.ones((4, 3)), host=host) == -1
            assert np.isnan(lv.read_all(40)).all() and np.isnan(lv.read_all(41)).all()
        assert B.call_combine(lv, [40], list(range(1, 38)), np.ones((37, 1))) == -1          # nin > 36
        assert B.call_combine(lv, list(range(20, 33)), [1], np.ones((1, 13))) == -1          # nout > 12
        assert B.call_combine(lv, [40], [48], np.ones((1, 1))) == -1                         # not a vector of the level
        assert B.call_gram(lv, list(range(1, 38)), [1], -1)[0] == -1 and B.call_gram(lv, [1], [48], -1)[0] == -1
        assert np.isnan(lv.read_all(40)).all()
    finally:
        B.write_fields(lv, F, [40, 41])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_residual_equals_the_restatement(bench_of, geom, weighted):
    lv, F = bench_of(geom)
    w = B.W_ID if weighted else -1
    nan = np.full((lv.num_boxes, lv.volume), np.nan)
    for name, (r_ids, ax_ids, x_ids) in B.residual_cases(geom).items():
        n = len(r_ids)
        mu = 0.5 + np.arange(n) * 0.75
        held = dict(F)
        for v in r_ids:
            held[v] = nan
        # column 0: the largest |r| sits in the last live lane of the last workgroup; the last column: the largest |w x| does
        box, cell = B.last_live_cell(lv)
        held[ax_ids[0]] = F[ax_ids[0]].copy(); held[ax_ids[0]][box, cell] = -HUGE
        held[x_ids[-1]] = F[x_ids[-1]].copy(); held[x_ids[-1]][box, cell] = HUGE
        touched = list(r_ids) + [ax_ids[0], x_ids[-1]]
        B.write_fields(lv, held, touched)
        try:
            rc, rmax, mxmax = B.call_residual(lv, r_ids, ax_ids, x_ids, w, mu)
            want, rmax_w, mxmax_w = B.residual_restated(lv, held, r_ids, ax_ids, x_ids, w, mu)
            assert rc == 0 and np.isfinite(rmax).all() and np.isfinite(mxmax).all()
            B.same_bits(rmax, rmax_w, f"{name} rmax"); B.same_bits(mxmax, mxmax_w, f"{name} mxmax")
            assert rmax[0] > 0.9 * HUGE and mxmax[-1] > 0.4 * HUGE and (n == 1 or (rmax[1:-1] < 20.0).all())
            q = cell_offsets(lv)
            for v in r_ids:
                got = lv.read_all(v)
                assert np.isfinite(got[:, q]).all()
                B.same_bits(got, want[v], f"{B.row_id(geom)} {name} r {v}")
            far = np.abs(want[r_ids[0]][:, q])
            assert np.unravel_index(far.argmax(), far.shape) == (box, lv.box_dim - 1, lv.box_dim - 1, lv.box_dim - 1)
        finally:
            B.write_fields(lv, F, touched)


def test_residual_skips_a_nan_and_refuses_shared_outputs(bench_of):
    """A NaN in x is never the maximum (norm()'s comparison); two columns may not write one vector, nor a column another column's input."""
    lv, F = bench_of((1, 20))
    x = F[2].copy()
    x[0, cell_offsets(lv)[3, 4, 5]] = np.nan
    lv.write_all(2, x)
    try:
        rc, rmax, mxmax = B.call_residual(lv, [30], [1], [2], -1, [1.5])
        assert rc == 0 and 0.0 < rmax[0] < 3.0 and 0.0 < mxmax[0] <= 1.0
        assert B.call_residual(lv, [30, 30], [1, 3], [2, 4], -1, [1.0, 1.0])[0] == -1
        assert B.call_residual(lv, [30, 3], [1, 3], [2, 4], -1, [1.0, 1.0])[0] == 0          # r_1 = ax_1: its own column
        assert B.call_residual(lv, [3, 31], [1, 3], [2, 4], -1, [1.0, 1.0])[0] == -1         # r_0 = ax_1: another column's input
    finally:
        B.write_fields(lv, F, [2, 3, 30, 31])
