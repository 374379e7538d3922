"""The block hooks of kernels/block.hip (hpgmg_block_gram / _combine / _residual) on the MI355X against the CPU oracle and the NumPy
restatements of tests/block_lib.py, as bit patterns: the rows, list sizes and cases of tests/test_oracle_block_hooks.py, on a HIP and an oracle level
that hold the same bytes.  Every ghost and padding double of every input is NaN and every output that is no input is pre-filled with NaN, so a kernel
that read or wrote outside the interior shows.  Every call asserts which form ran: 1 = the kernel on HIP, 0 = the portable form on the oracle -- and,
on a level the kernels do not take (constant coefficients; ghost-free mode off: the PORTABLE rows of tests/test_gpu_pcg_passes.py), 0 on HIP too.

| level (boxes per side, side) | ncb x nseg x boxes = items | what only this reaches |
|---|---|---|
| (1, 4) | 1 | 16 live columns of 256, one segment of 4 planes (one 4-plane chunk of block_combine) |
| (1, 12) | 1 | one ragged segment of 12 planes |
| (1, 20) | 2 x 2 = 4 | a block starting mid-row; a second segment of 4 planes |
| (3, 12) | 27 | many boxes in the fold |
| (2, 24) | 3 x 2 x 8 = 48 | 64 live columns in the last block; a last segment of 8 planes |
| (1, 40) | 7 x 3 = 21 | three segments |
| (17, 4) | 4913 | the in-place fold of block_fold_kernel: chunk 8, 615 lanes, the last owns 1 |
"""
import ctypes

import numpy as np
import pytest

import block_lib as B
import hpgmg_amd as H
import hpgmg_testlib as T
import pcg_lib as P
from reduction_lib import HUGE, cell_offsets

pytestmark = pytest.mark.gpu
PORTABLE_ROWS = [(3, 12), (1, 20)]
_kept = {}


@pytest.fixture(scope="module", autouse=True)
def _module(hip, oracle):
    hip.lib.hpgmg_set_ghost_free.argtypes = [ctypes.c_int]
    hip.lib.hpgmg_set_ghost_free(1)
    assert H.load_kernels().hpgmg_hip_block_tile() == B.TILE
    yield
    while _kept:
        for lv in _kept.popitem()[1][:2]:
            lv.destroy()
    for be in (hip, oracle):
        be.configure(**T.VARIANTS["7pt-cheby-helm"])


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom, variant): (HIP level, oracle level, fields) of one row, made once for the module under the configuration named."""
    def get(geom, variant="7pt-cheby-helm"):
        for be in (hip, oracle):
            be.configure(**T.VARIANTS[variant])
        if (geom, variant) not in _kept:
            P.check_row(geom)
            lh, lo = B.new_level(hip, geom), B.new_level(oracle, geom)
            F = B.fields_of(lo, 900 + 13 * geom[0] + geom[1])
            B.write_fields(lh, F); B.write_fields(lo, F)
            _kept[geom, variant] = (lh, lo, F)
        return _kept[geom, variant]
    return get


def gram_checks(lh, lo, F, geom, w, took, cases=None):
    for name, (a, b) in B.gram_cases(geom).items():
        if cases is not None and name not in cases:
            continue
        (rc_h, G_h), (rc_o, G_o) = B.call_gram(lh, a, b, w), B.call_gram(lo, a, b, w)
        assert (rc_h, rc_o) == (took, 0) and np.isfinite(G_h).all(), (name, rc_h, rc_o)
        B.same_bits(G_h, G_o, f"{B.row_id(geom)} {name}: HIP against the oracle")
        B.same_bits(G_h, B.gram_restated(lo, F, a, b, w), f"{B.row_id(geom)} {name}: HIP against the restatement")
        if w < 0:
            i, j = len(a) - 1, len(b) - 1
            t, value = P.call_dot(lh, a[i], b[j])
            assert t == took and P.same_scalar(G_h[i, j], value), (name, G_h[i, j], value)


def combine_checks(lh, lo, F, geom, took, cases=None):
    nan = np.full((lo.num_boxes, lo.volume), np.nan)
    q = cell_offsets(lo)
    for n, (name, (out_ids, in_ids, zero)) in enumerate(B.combine_cases(geom).items()):
        if cases is not None and name not in cases:
            continue
        C = B.combine_matrix(len(in_ids), len(out_ids), zero, 40 + n)
        held = dict(F)
        for v in out_ids:
            if v not in in_ids:
                held[v] = nan
        try:
            for lv in (lh, lo):
                B.write_fields(lv, held, out_ids)
            assert (B.call_combine(lh, out_ids, in_ids, C), B.call_combine(lo, out_ids, in_ids, C)) == (took, 0), name
            want = B.combine_restated(lo, held, out_ids, in_ids, C)
            for v in out_ids:
                got = lh.read_all(v)
                assert np.isfinite(got[:, q]).all(), (name, v)
                B.same_bits(got, lo.read_all(v), f"{B.row_id(geom)} {name} output {v}: HIP against the oracle")
                B.same_bits(got, want[v], f"{B.row_id(geom)} {name} output {v}: HIP against the restatement")
            for v in in_ids:
                if v not in out_ids:
                    B.same_bits(lh.read_all(v), F[v], f"{name} input {v}")
        finally:
            for lv in (lh, lo):
                B.write_fields(lv, F, out_ids)


def residual_checks(lh, lo, F, geom, w, took):
    nan = np.full((lo.num_boxes, lo.volume), np.nan)
    for name, (r_ids, ax_ids, x_ids) in B.residual_cases(geom).items():
        n = len(r_ids)
        mu = 0.5 + np.arange(n) * 0.75
        held = dict(F)
        for v in r_ids:
            held[v] = nan
        box, cell = B.last_live_cell(lo)          # the planted maxima meet the last live lane of the last workgroup last
        held[ax_ids[0]] = F[ax_ids[0]].copy(); held[ax_ids[0]][box, cell] = -HUGE
        held[x_ids[-1]] = F[x_ids[-1]].copy(); held[x_ids[-1]][box, cell] = HUGE
        touched = list(r_ids) + [ax_ids[0], x_ids[-1]]
        try:
            for lv in (lh, lo):
                B.write_fields(lv, held, touched)
            (rc_h, rmax_h, mx_h), (rc_o, rmax_o, mx_o) = B.call_residual(lh, r_ids, ax_ids, x_ids, w, mu), B.call_residual(lo, r_ids, ax_ids, x_ids, w, mu)
            want, rmax_w, mx_w = B.residual_restated(lo, held, r_ids, ax_ids, x_ids, w, mu)
            assert (rc_h, rc_o) == (took, 0), name
            print(f"{B.row_id(geom)} residual {name}: rmax hip {rmax_h[0]!r} oracle {rmax_o[0]!r}; mxmax hip {mx_h[-1]!r} oracle {mx_o[-1]!r}")
            B.same_bits(rmax_h, rmax_o, "rmax: HIP against the oracle"); B.same_bits(mx_h, mx_o, "mxmax: HIP against the oracle")
            B.same_bits(rmax_h, rmax_w, "rmax: HIP against the restatement"); B.same_bits(mx_h, mx_w, "mxmax: HIP against the restatement")
            assert rmax_h[0] > 0.9 * HUGE and mx_h[-1] > 0.4 * HUGE
            for v in r_ids:
                got = lh.read_all(v)
                B.same_bits(got, lo.read_all(v), f"{B.row_id(geom)} {name} r {v}: HIP against the oracle")
                B.same_bits(got, want[v], f"{B.row_id(geom)} {name} r {v}: HIP against the restatement")
        finally:
            for lv in (lh, lo):
                B.write_fields(lv, F, touched)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_gram_equals_the_oracle(pair_of, geom, weighted):
    lh, lo, F = pair_of(geom)
    gram_checks(lh, lo, F, geom, B.W_ID if weighted else -1, took=1)


@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_combine_equals_the_oracle(pair_of, geom):
    lh, lo, F = pair_of(geom)
    combine_checks(lh, lo, F, geom, took=1)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("geom", B.ROWS, ids=B.row_id)
def test_residual_equals_the_oracle(pair_of, geom, weighted):
    lh, lo, F = pair_of(geom)
    residual_checks(lh, lo, F, geom, B.W_ID if weighted else -1, took=1)


def test_refusals_launch_nothing(pair_of):
    lh, lo, F = pair_of((1, 12))
    nan = np.full((lh.num_boxes, lh.volume), np.nan)
    B.write_fields(lh, {40: nan, 41: nan})
    try:
        assert B.call_combine(lh, [40, 41, 40], [1, 2, 3, 4], np.ones((4, 3))) == -1
        assert B.call_combine(lh, [40], list(range(1, 38)), np.ones((37, 1))) == -1 and B.call_combine(lh, [40], [48], np.ones((1, 1))) == -1
        assert B.call_gram(lh, list(range(1, 38)), [1], -1)[0] == -1 and B.call_gram(lh, [1], [48], -1)[0] == -1
        assert B.call_residual(lh, [40, 40], [1, 3], [2, 4], -1, [1.0, 1.0])[0] == -1 and B.call_residual(lh, [3, 41], [1, 3], [2, 4], -1, [1.0, 1.0])[0] == -1
        assert np.isnan(lh.read_all(40)).all() and np.isnan(lh.read_all(41)).all()
        B.same_bits(lh.read_all(3), F[3], "an input of a refused call")
    finally:
        B.write_fields(lh, F, [40, 41])


# ---------------------------------------------------------------------------------------------------------------- the portable forms, as the HIP build runs them
SOME_GRAMS = ["identical-13", f"{B.TILE + 1}x{B.TILE - 1}", f"{B.TILE - 1}x{B.TILE + 1}-overlap"]
SOME_COMBINES = ["alias-7-to-5", "36-to-12-disjoint"]


@pytest.mark.parametrize("geom", PORTABLE_ROWS, ids=B.row_id)
def test_portable_forms_on_constant_coefficients(pair_of, geom):
    """7ptcc-cheby is not a level the kernels take: the plugin runs the host layer's portable forms on downloaded boxes and returns 0."""
    lh, lo, F = pair_of(geom, "7ptcc-cheby")
    gram_checks(lh, lo, F, geom, B.W_ID, took=0, cases=SOME_GRAMS)
    gram_checks(lh, lo, F, geom, -1, took=0, cases=SOME_GRAMS)
    combine_checks(lh, lo, F, geom, took=0, cases=SOME_COMBINES)
    residual_checks(lh, lo, F, geom, B.W_ID, took=0)


@pytest.mark.parametrize("geom", PORTABLE_ROWS, ids=B.row_id)
def test_portable_forms_with_ghost_free_mode_off(hip, pair_of, geom):
    lh, lo, F = pair_of(geom)
    hip.lib.hpgmg_set_ghost_free(0)
    try:
        gram_checks(lh, lo, F, geom, -1, took=0, cases=SOME_GRAMS)
        combine_checks(lh, lo, F, geom, took=0, cases=SOME_COMBINES)
        residual_checks(lh, lo, F, geom, -1, took=0)
    finally:
        hip.lib.hpgmg_set_ghost_free(1)
