"""The four CG passes of include/hpgmg_operators.h (hpgmg_pcg_apply_dot / _update / _dot / _dot2) on the CPU oracle, called on
plain levels pass by pass: the portable forms of host/hooks_host.inc must equal the restatement of the header's one summation order in
tests/pcg_lib.py bit for bit at every geometry of pcg_lib.TABLE -- the geometries tests/test_gpu_pcg_passes.py then holds kernels/pcg.hip to.

The restatement is only worth that if the data can tell one order from another, so three wrong statements of the order (columns numbered
c = j + dim i, segments of 8 planes, no tree below a workgroup's 256 leaves) must each give other bits on the geometries that target them.  And the
claim the kernels rely on -- a value of the tree is never -0.0, so folding more zero padding than the header names changes no bit -- is checked where
it could fail: every product -0.0, and every product underflowing to -0.0.
"""
import numpy as np
import pytest

import hpgmg_testlib as T
import pcg_lib as P
from reduction_lib import bits, cell_offsets, random_field

_levels = {}


@pytest.fixture(scope="module")
def level_of():
    """level_of(geom, periodic): the oracle's level of one row, coefficients set, made once for the module."""
    be = T.Backend.oracle()

    def get(geom, periodic=False):
        be.configure(**T.VARIANTS["7pt-cheby-helm"])
        if (geom, periodic) not in _levels:
            lv = P.new_level(be, geom, periodic)
            P.coefficient_fields(lv, 500 + geom[1])
            _levels[geom, periodic] = lv
        return _levels[geom, periodic]
    yield get
    while _levels:
        _levels.popitem()[1].destroy()


def fill(lv, seed, names=("x", "r", "z", "p", "Ap")):
    data = {name: random_field(lv, seed + n) for n, name in enumerate(names)}
    for name, f in data.items():
        lv.write_all(P.IDS[name], f)
    return data


@pytest.mark.parametrize("variant", sorted(P.VARIANTS))
@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_each_pass_equals_the_restatement(level_of, row, variant):
    geom, periodic = row
    P.check_row(geom)
    lv = level_of(geom, periodic)
    lv.b.configure(**T.VARIANTS[variant])
    a, b = P.VARIANTS[variant]
    data = fill(lv, 7 * geom[0] + geom[1])
    lv.write_all(P.IDS["Ap"], np.full_like(data["Ap"], np.nan))
    out = P.run_passes(lv, a, b)
    assert set(out["took"].values()) == {0}
    # apply_dot: the oracle's own apply_op, then the restated sum over p . Ap
    lv.b.lib.apply_op(lv.ptr, P.IDS["spare"], P.IDS["p"], a, b)
    q = cell_offsets(lv)
    assert np.array_equal(bits(out["Ap"][:, q]), bits(lv.read_all(P.IDS["spare"])[:, q])) and not np.isnan(out["Ap"][:, q]).any()
    outside = np.ones(lv.volume, dtype=bool)
    outside[q.ravel()] = False
    assert np.isnan(out["Ap"][:, outside]).all()                              # no cell outside the interior was written
    assert P.same_scalar(out["pAp"], P.dot(lv, out["p"], out["Ap"])) and out["pAp"] != 0.0
    # update
    x, r, rmax = P.update(lv, data["x"], data["r"], out["p"], out["Ap"], P.ALPHA_CG)
    assert np.array_equal(bits(out["x"]), bits(x)) and np.array_equal(bits(out["r"]), bits(r)) and P.same_scalar(out["rmax"], rmax)
    # dot, dot2
    assert P.same_scalar(out["rz"], P.dot(lv, r, data["z"])) and P.same_scalar(out["Apz"], P.dot(lv, out["Ap"], data["z"]))
    assert P.same_scalar(out["rz2"], out["rz"]) and P.same_scalar(out["Apz2"], out["Apz"])
    assert len({out["rz"], out["Apz"], out["pAp"], 0.0}) == 4


# the three wrong orders, each with the geometries that target it (and (1, 1), where every order is the one product)
WRONG = {"column-major": (dict(column_major=True), [(1, 12), (1, 20), (3, 12), (1, 104)]),
         "segment-of-8": (dict(segment=8), [(1, 12), (1, 20), (2, 24), (1, 40)]),
         "no-leaf-tree": (dict(leaf_tree=False), [(1, 4), (1, 12), (1, 64), (17, 4)])}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_the_data_can_tell_a_wrong_order(level_of, name):
    """Three sums per geometry (r . z, x . z, p . z: two orders of one sum agree in about one draw of three, the last bit being all they differ in)."""
    wrong, geoms = WRONG[name]
    for geom in geoms + [(1, 1)]:
        lv = level_of(geom)
        data = fill(lv, 7 * geom[0] + geom[1], names=("r", "x", "p", "z"))
        values, others = [], []
        for a in ("r", "x", "p"):
            took, value = P.call_dot(lv, a, "z")
            assert took == 0 and P.same_scalar(value, P.dot(lv, data[a], data["z"]))
            values.append(value)
            others.append(P.dot(lv, data[a], data["z"], **wrong))
            assert abs(others[-1] - value) <= 1e-13 * geom[0] ** 3 * geom[1] ** 3          # the same sum, in another order
        assert (others == values) == (geom == (1, 1)), (name, geom, values, others)


def sign_bit_clear(v):
    return v == 0.0 and not np.signbit(v)


@pytest.mark.parametrize("a_value,b_value", [(-0.0, 1.0), (-1e-200, 1e-200)], ids=["minus-zero", "underflow"])
@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_a_sum_of_negative_zeros_is_plus_zero(level_of, row, a_value, b_value):
    """Every product is -0.0 (a = -0.0; or a b = -1e-400, which underflows): every chain starts 0.0 + (-0.0) = +0.0, so the sums are +0.0."""
    geom, periodic = row
    lv = level_of(geom, periodic)
    ones = np.ones((lv.num_boxes, lv.volume))
    assert np.signbit(a_value * b_value) and a_value * b_value == 0.0
    for name, value in (("r", a_value), ("p", a_value), ("Ap", a_value), ("z", b_value)):
        lv.write_all(P.IDS[name], value * ones)
    assert np.signbit(lv.read_all(P.IDS["r"])).all()
    got = [P.call_dot(lv, "r", "z")[1], *P.call_dot2(lv, "r", "Ap", "z")[1:], P.call_apply_dot(lv, "spare", "p", 1.3, 0.9)[1]]
    want = [P.dot(lv, a_value * ones, b_value * ones)] * 3 + [P.dot(lv, lv.read_all(P.IDS["p"]), lv.read_all(P.IDS["spare"]))]
    assert all(sign_bit_clear(v) for v in got + want), (got, want)
