"""The three hooks of the Newmark march (include/hpgmg_operators.h hpgmg_wave_predict / _correct / _init) on the CPU oracle, on plain
levels: the portable forms of host/hooks_host.inc must equal the NumPy restatements of tests/user_wave_lib.py as 64-bit patterns over whole padded boxes
-- every ghost and padding double of every vector is NaN, and every vector a pass only writes is NaN throughout -- and as bits in the two sums, at every
row of pcg_lib.ROWS: the rows tests/test_gpu_wave_hooks.py then holds kernels/dense_wave.hip to.  The kinetic sum is hpgmg_block_gram([v], [v], alpha),
bit for bit, and the data can tell a wrong summation order apart.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import hpgmg_testlib as T
import pcg_lib as P
import user_wave_lib as W
from reduction_lib import cell_offsets

_kept = {}
CU, CV, A, CQ, CG = W.coefficients_of(W.HOOK_DT, W.HOOK_BETA, W.HOOK_GAMMA, W.HOOK_SIGMA)


@pytest.fixture(scope="module")
def bench_of():
    """bench_of(row): (level, fields) of one row on the oracle, made once for the module; the level holds the fields."""
    be = T.Backend.oracle()
    be.configure(**T.VARIANTS["7pt-cheby-helm"])

    def get(row):
        if row not in _kept:
            geom, periodic = row
            P.check_row(geom)
            lv = W.new_level(be, geom, periodic)
            F = W.fields_of(lv, 700 + 13 * geom[0] + geom[1])
            W.write_fields(lv, F)
            _kept[row] = (lv, F)
        return _kept[row]
    yield get
    while _kept:
        _kept.popitem()[1][0].destroy()


def _nan(lv):
    return np.full((lv.num_boxes, lv.volume), np.nan)


def _gram_vv(lv):
    ids = (ctypes.c_int * 1)(W.IDS["v"])
    G = (ctypes.c_double * 1)(np.nan)
    assert lv.b.lib.hpgmg_block_gram(lv.ptr, ids, 1, ids, 1, W.ALPHA, G) == 0
    return G[0]


@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_predict_equals_the_restatement(bench_of, row):
    lv, F = bench_of(row)
    held = dict(F, uold=_nan(lv))
    try:
        W.write_fields(lv, held, ["uold"])
        assert W.call_predict(lv, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA) == 0
        want = W.predict_restated(lv, held, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA)
        c = cell_offsets(lv)
        for name in ("u", "uold", "v", "F"):
            got = lv.read_all(W.IDS[name])
            assert np.isfinite(got[:, c]).all(), name
            W.same_bits(got, want[name], f"{P.row_id(row)} {name}")
        W.same_bits(lv.read_all(W.IDS["q"]), F["q"], "q, an input")
        W.same_bits(lv.read_all(W.ALPHA), F["alpha"], "alpha, an input")
    finally:
        W.write_fields(lv, F, ["u", "uold", "v", "F"])


@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_correct_equals_the_restatement_and_block_gram(bench_of, row):
    lv, F = bench_of(row)
    held = dict(F, q=_nan(lv))
    try:
        W.write_fields(lv, held, ["q"])
        rc, sums = W.call_correct(lv, A, CQ, CG)
        want, want_sums = W.correct_restated(lv, held, A, CQ, CG)
        assert rc == 0 and np.isfinite(sums).all()
        for name in ("q", "v"):
            W.same_bits(lv.read_all(W.IDS[name]), want[name], f"{P.row_id(row)} {name}")
        W.same_sums(sums, want_sums, P.row_id(row))
        assert P.same_scalar(sums[0], _gram_vv(lv)), "the kinetic sum is hpgmg_block_gram([v], [v], alpha) on the new v"
        for name in ("u", "uold", "F", "r"):
            W.same_bits(lv.read_all(W.IDS[name]), F[name], f"{name}, an input")
    finally:
        W.write_fields(lv, F, ["q", "v"])


@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_init_equals_the_restatement_and_block_gram(bench_of, row):
    lv, F = bench_of(row)
    held = dict(F, q=_nan(lv))
    try:
        W.write_fields(lv, held, ["q"])
        rc, sums = W.call_init(lv, A, W.HOOK_SIGMA)
        want, want_sums = W.init_restated(lv, held, A, W.HOOK_SIGMA)
        assert rc == 0 and np.isfinite(sums).all()
        W.same_bits(lv.read_all(W.IDS["q"]), want["q"], f"{P.row_id(row)} q")
        W.same_sums(sums, want_sums, P.row_id(row))
        assert P.same_scalar(sums[0], _gram_vv(lv))
        for name in ("u", "v", "F", "r"):
            W.same_bits(lv.read_all(W.IDS[name]), F[name], f"{name}, an input")
        assert W.call_init(lv, A, W.HOOK_SIGMA, host=True)[0] == 0
    finally:
        W.write_fields(lv, F, ["q"])


@pytest.mark.parametrize("wrong", [dict(segment=8), dict(column_major=True)], ids=["segments-of-8", "columns-j-major"])
def test_a_wrong_order_is_told_apart(bench_of, wrong):
    """At 2 x 24 (two segments, three column blocks) the sums of another order have other bits: the restatement pins the order, not just the value."""
    lv, F = bench_of(((2, 24), False))
    try:
        rc, sums = W.call_init(lv, A, W.HOOK_SIGMA)
        _, right = W.init_restated(lv, F, A, W.HOOK_SIGMA)
        _, other = W.init_restated(lv, F, A, W.HOOK_SIGMA, **wrong)
        W.same_sums(sums, right, "the header's order")
        assert np.allclose(other, right, rtol=1e-12, atol=0) and not (P.same_scalar(other[0], right[0]) and P.same_scalar(other[1], right[1]))
    finally:
        W.write_fields(lv, F, ["q"])


def test_refusals_write_nothing(bench_of):
    lv, F = bench_of(((1, 12), False))
    held = dict(F, q=_nan(lv), uold=_nan(lv))
    try:
        W.write_fields(lv, held, ["q", "uold"])
        for ids in (dict(u=W.VECTORS), dict(q=-1), dict(uold=W.IDS["u"]), dict(F=W.IDS["v"]), dict(v=W.ALPHA), dict(q=W.IDS["u"])):
            assert W.call_predict(lv, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA, ids=ids) == -1, ids
        for ids in (dict(r=W.VECTORS), dict(q=W.IDS["v"]), dict(q=W.IDS["r"]), dict(v=W.IDS["uold"]), dict(q=W.ALPHA)):
            assert W.call_correct(lv, A, CQ, CG, ids=ids)[0] == -1, ids
        for ids in (dict(F=-3), dict(q=W.IDS["u"]), dict(q=W.IDS["F"]), dict(q=W.ALPHA)):
            assert W.call_init(lv, A, W.HOOK_SIGMA, ids=ids)[0] == -1, ids
        for name in W.IDS:
            W.same_bits(lv.read_all(W.IDS[name]), held[name], name)
        assert W.call_correct(lv, A, CQ, CG, ids=dict(F=W.IDS["r"]))[0] == 0          # two inputs may be one vector
    finally:
        W.write_fields(lv, F)


def test_a_level_without_alpha_is_refused():
    be = T.Backend.oracle()
    be.configure(**T.VARIANTS["7pt-cheby-helm"])
    lv = be.level(1, 4, num_vectors=H.VECTOR_ALPHA)          # ids 0 .. VECTOR_ALPHA - 1: no alpha
    try:
        assert lv.b.lib.hpgmg_wave_predict(lv.ptr, 0, 1, 2, 3, 4, 0.1, 0.1, 0.1, 1.0, 0.0) == -1
    finally:
        lv.destroy()
