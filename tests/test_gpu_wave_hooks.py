"""The three passes of kernels/dense_wave.hip (hpgmg_wave_predict / _correct / _init) on the MI355X against the CPU oracle and the NumPy
restatements of tests/user_wave_lib.py, as bit patterns over whole padded boxes and in the two sums: the rows of pcg_lib.ROWS (the table of
tests/test_gpu_pcg_passes.py: one live lane, ragged segments, a block starting mid-row, many boxes, the in-place strides of the fold launch, the periodic
wrap), on a HIP and an oracle level that hold the same bytes.  Every ghost and padding double is NaN and every vector a pass only writes is NaN
throughout, so a kernel that read or wrote outside the interior shows.  Every call asserts which form ran: 1 = the kernel on HIP, 0 = the portable form
on the oracle.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import hpgmg_testlib as T
import pcg_lib as P
import user_wave_lib as W
from reduction_lib import cell_offsets

pytestmark = pytest.mark.gpu
_kept = {}
CU, CV, A, CQ, CG = W.coefficients_of(W.HOOK_DT, W.HOOK_BETA, W.HOOK_GAMMA, W.HOOK_SIGMA)


@pytest.fixture(scope="module", autouse=True)
def _module(hip, oracle):
    hip.lib.hpgmg_set_ghost_free.argtypes = [ctypes.c_int]
    hip.lib.hpgmg_set_ghost_free(1)
    yield
    while _kept:
        for lv in _kept.popitem()[1][:2]:
            lv.destroy()
    for be in (hip, oracle):
        be.configure(**T.VARIANTS["7pt-cheby-helm"])


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(row): (HIP level, oracle level, fields) of one row, made once for the module."""
    def get(row):
        for be in (hip, oracle):
            be.configure(**T.VARIANTS["7pt-cheby-helm"])
        if row not in _kept:
            geom, periodic = row
            P.check_row(geom)
            lh, lo = W.new_level(hip, geom, periodic), W.new_level(oracle, geom, periodic)
            F = W.fields_of(lo, 700 + 13 * geom[0] + geom[1])
            W.write_fields(lh, F); W.write_fields(lo, F)
            _kept[row] = (lh, lo, F)
        return _kept[row]
    return get


def _nan(lv):
    return np.full((lv.num_boxes, lv.volume), np.nan)


def _load(lh, lo, held, names):
    for lv in (lh, lo):
        W.write_fields(lv, held, names)


def predict_check(lh, lo, F, what):
    held = dict(F, uold=_nan(lo))
    try:
        _load(lh, lo, held, ["uold"])
        rcs = [W.call_predict(lv, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA) for lv in (lh, lo)]
        assert rcs == [1, 0], (what, rcs)
        want = W.predict_restated(lo, held, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA)
        for name in ("u", "uold", "v", "F"):
            got = lh.read_all(W.IDS[name])
            W.same_bits(got, lo.read_all(W.IDS[name]), f"{what} {name}: HIP against the oracle")
            W.same_bits(got, want[name], f"{what} {name}: HIP against the restatement")
        W.same_bits(lh.read_all(W.IDS["q"]), F["q"], "q, an input")
    finally:
        _load(lh, lo, F, ["u", "uold", "v", "F"])


def sums_check(lh, lo, F, what, which, finite=True):
    """wave_correct (which = "correct") or wave_init on both levels from the fields F with q pre-filled with NaN."""
    held = dict(F, q=_nan(lo))
    try:
        _load(lh, lo, held, ["q"])
        if which == "correct":
            (rc_h, s_h), (rc_o, s_o) = [W.call_correct(lv, A, CQ, CG) for lv in (lh, lo)]
            want, s_w = W.correct_restated(lo, held, A, CQ, CG)
        else:
            (rc_h, s_h), (rc_o, s_o) = [W.call_init(lv, A, W.HOOK_SIGMA) for lv in (lh, lo)]
            want, s_w = W.init_restated(lo, held, A, W.HOOK_SIGMA)
        print(f"{what} {which}: sums hip {s_h!r} oracle {s_o!r}")
        assert (rc_h, rc_o) == (1, 0), (what, rc_h, rc_o)
        assert np.isfinite(s_h).all() == finite, (what, s_h)
        for name in want:
            got = lh.read_all(W.IDS[name])
            W.same_bits(got, lo.read_all(W.IDS[name]), f"{what} {which} {name}: HIP against the oracle")
            W.same_bits(got, want[name], f"{what} {which} {name}: HIP against the restatement")
        W.same_sums(s_h, s_o, f"{what} {which}: HIP against the oracle")
        W.same_sums(s_h, s_w, f"{what} {which}: HIP against the restatement")
        for name in ("u", "uold", "F", "r"):
            W.same_bits(lh.read_all(W.IDS[name]), F[name], f"{name}, an input")
        return s_h
    finally:
        _load(lh, lo, F, ["q", "v"])


@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_the_three_passes_equal_the_oracle(pair_of, row):
    lh, lo, F = pair_of(row)
    predict_check(lh, lo, F, P.row_id(row))
    sums_check(lh, lo, F, P.row_id(row), "correct")
    sums_check(lh, lo, F, P.row_id(row), "init")


def test_after_a_larger_level_has_used_the_scratch(pair_of):
    """9261 and 4913 workgroup values per sum, then 1 and 4 on the same scratch: what the larger launches left past the smaller ones' values enters no sum."""
    for row in (((21, 4), False), ((1, 1), False), ((17, 4), False), ((1, 20), False)):
        lh, lo, F = pair_of(row)
        sums_check(lh, lo, F, P.row_id(row), "correct")
        sums_check(lh, lo, F, P.row_id(row), "init")


@pytest.mark.parametrize("row", [((2, 24), False), ((1, 20), False)], ids=P.row_id)
def test_an_inf_in_the_last_cell_propagates(pair_of, row):
    """One Inf in u in the last cell of the last box: the last live lane of the last workgroup meets it last.  No special rule: both sums take it as the
    oracle's do (the potential term u (.. - (a alpha) u) is -Inf there; wave_correct's new v, and with it the kinetic term, is Inf)."""
    lh, lo, F = pair_of(row)
    d = lo.box_dim
    spoiled = dict(F, u=F["u"].copy())
    spoiled["u"][lo.num_boxes - 1, int(cell_offsets(lo)[d - 1, d - 1, d - 1])] = np.inf
    try:
        _load(lh, lo, spoiled, ["u"])
        s = sums_check(lh, lo, spoiled, P.row_id(row), "init", finite=False)
        assert np.isfinite(s[0]) and not np.isfinite(s[1])
        sums_check(lh, lo, spoiled, P.row_id(row), "correct", finite=False)
    finally:
        _load(lh, lo, F, ["u"])


def test_refused_hooks_write_nothing(pair_of):
    lh, lo, F = pair_of(((1, 12), False))
    held = dict(F, q=_nan(lh), uold=_nan(lh))
    try:
        W.write_fields(lh, held, ["q", "uold"])
        for ids in (dict(u=W.VECTORS), dict(q=-1), dict(uold=W.IDS["u"]), dict(F=W.IDS["v"]), dict(v=W.ALPHA), dict(q=W.IDS["u"])):
            assert W.call_predict(lh, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA, ids=ids) == -1, ids
        for ids in (dict(r=W.VECTORS), dict(q=W.IDS["v"]), dict(q=W.IDS["r"]), dict(v=W.IDS["uold"]), dict(q=W.ALPHA)):
            assert W.call_correct(lh, A, CQ, CG, ids=ids)[0] == -1, ids
        for ids in (dict(F=-3), dict(q=W.IDS["u"]), dict(q=W.IDS["F"]), dict(q=W.ALPHA)):
            assert W.call_init(lh, A, W.HOOK_SIGMA, ids=ids)[0] == -1, ids
        for name in W.IDS:
            W.same_bits(lh.read_all(W.IDS[name]), held[name], name)
    finally:
        W.write_fields(lh, F, ["q", "uold"])


def test_the_launchers_refuse_before_they_launch():
    """hpgmg_hip_wave_*: an id outside the level's vectors, a written vector named twice or equal to alpha, a level without alpha and a geometry the mapping
    does not hold are refused with an error code and sums of 0.0.  The level is hand-built: its device pointers are null, and no call here is accepted."""
    K = H.load_kernels()
    lvl = H.HipLevel()
    lvl.dim, lvl.ghosts, lvl.jStride, lvl.kStride, lvl.volume, lvl.num_boxes = 8, 1, 10, 100, 1000, 1
    p = ctypes.byref(lvl)
    u, uold, v, F, q, r, nv = W.IDS["u"], W.IDS["uold"], W.IDS["v"], W.IDS["F"], W.IDS["q"], W.IDS["r"], W.VECTORS

    def predict(nv, *ids):
        return K.hpgmg_hip_wave_predict(p, nv, *ids, W.HOOK_DT, CU, CV, A, W.HOOK_SIGMA)

    def correct(nv, *ids):
        s = (ctypes.c_double * 2)(-1.0, -1.0)
        st = K.hpgmg_hip_wave_correct(p, nv, *ids, A, CQ, CG, s)
        assert (s[0], s[1]) == (0.0, 0.0)
        return st

    def init(nv, *ids):
        s = (ctypes.c_double * 2)(-1.0, -1.0)
        st = K.hpgmg_hip_wave_init(p, nv, *ids, A, W.HOOK_SIGMA, s)
        assert (s[0], s[1]) == (0.0, 0.0)
        return st

    for ids in [(u, u, v, F, q), (u, uold, u, F, q), (u, uold, v, v, q), (u, uold, v, F, u), (W.ALPHA, uold, v, F, q), (u, uold, v, F, nv), (-1, uold, v, F, q)]:
        assert predict(nv, *ids) != 0, ids
    for ids in [(q, q, u, uold, F, r), (q, v, q, uold, F, r), (q, v, u, v, F, r), (W.ALPHA, v, u, uold, F, r), (q, v, u, uold, F, nv + 50)]:
        assert correct(nv, *ids) != 0, ids
    for ids in [(r, r, u, v, F), (u, r, u, v, F), (q, r, u, v, -1), (W.ALPHA, r, u, v, F)]:
        assert init(nv, *ids) != 0, ids
    for few in (H.VECTOR_ALPHA, 0):                                          # no alpha vector
        assert predict(few, 1, 2, 3, 4, 5) != 0 and correct(few, 1, 2, 3, 4, 5, 0) != 0 and init(few, 1, 0, 2, 3, 4) != 0
    lvl.num_boxes = 0                                                        # good ids, a level the mapping does not hold
    assert predict(nv, u, uold, v, F, q) != 0 and correct(nv, q, v, u, uold, F, r) != 0 and init(nv, q, r, u, v, F) != 0
    lvl.num_boxes, lvl.dim = 1, 2048
    assert predict(nv, u, uold, v, F, q) != 0 and correct(nv, q, v, u, uold, F, r) != 0 and init(nv, q, r, u, v, F) != 0
