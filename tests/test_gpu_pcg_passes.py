"""The CG passes of kernels/pcg.hip alone, at the edges of their launch shape (DESIGN.md §11.3 "The passes alone"): hpgmg_pcg_apply_dot, _update, _dot
and _dot2 called pass by pass on plain levels of 14 vectors -- no Solver, so any (boxes per side, box side) -- on the MI355X and on the CPU oracle,
whose portable forms tests/test_oracle_pcg_passes.py holds to the NumPy restatement of the header's order (tests/pcg_lib.py).  Everything is compared
bit for bit: the vectors as uint64 over whole padded boxes (every output pre-filled with NaN on both sides, so a cell written outside the interior
or not written shows), the scalars as bits.  Only the operand p is compared on the interior alone: its ghost zones are scratch in ghost-free mode,
while the oracle's apply_op fills them.  Every call asserts which form ran (1 = the kernel on HIP, 0 = the portable form on the oracle) and its row
of the table against the launch arithmetic restated in pcg_lib (pcg_items, pcg_fold_plan):

| level (boxes per side, side) | ncb x nseg x boxes = items | fold | what only this reaches |
|---|---|---|---|
| (1, 1) | 1 | n = 1 | one live lane, six Dirichlet faces on one cell |
| (1, 4) | 1 | n = 1 | Solver's smallest box: 16 live columns |
| (1, 12) | 1 | | one ragged segment of 12 planes |
| (1, 20) | 2 x 2 = 4 | | a block starting mid-row (256 = 12 * 20 + 16); last block has 144 live; second segment has 4 planes; `above` in-column for segment 0, across the face for segment 1 |
| (3, 12) | 27 | | a box on no wall: all six neighbours from box_nbr |
| (2, 24) | 3 x 2 x 8 = 48 | | last block has 64 live columns; short last segment next to a neighbouring box |
| (1, 40) | 7 x 3 = 21 | | three segments, with the middle one full |
| (1, 64) | 16 x 4 = 64 | | a power-of-two side the pass tests of the Solver files skip |
| (1, 104) | 43 x 7 = 301 | | rows longer than a wave that straddle blocks |
| (15, 4) | 3375 | chunk 4, 844 lanes, last owns 3 | ragged end inside a chunk |
| (17, 4) | 4913 | chunk 8, 615 lanes, last owns 1 | Solver(68, box_dim=4) |
| (21, 4) | 9261 | chunk 16, 579 lanes, last owns 13 | four in-place strides |
| (1, 12) and (2, 24), periodic | | | a box that is its own neighbour; the wrap |

Unheld per pass: sides of 256 and above (4096 values are reached by dot2 at (2, 128) in tests/test_gpu_reductions.py; a 512^3 box is 15 GB) and the
multi-rank hp_allreduce_scalar.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import hpgmg_testlib as T
import pcg_lib as P
from reduction_lib import HUGE, bits, cell_offsets, random_field

pytestmark = pytest.mark.gpu
_kept = {}


@pytest.fixture(scope="module", autouse=True)
def _module(hip, oracle):
    hip.lib.hpgmg_set_ghost_free.argtypes = [ctypes.c_int]
    hip.lib.hpgmg_set_ghost_free(1)
    yield
    while _kept:
        _kept.popitem()[1].destroy()
    for be in (hip, oracle):
        be.configure(**T.VARIANTS["7pt-cheby-helm"])


def configure(hip, oracle, variant):
    for be in (hip, oracle):
        be.configure(**T.VARIANTS[variant])


class Pair:
    """The HIP and the oracle level of one row: the same coefficient bytes (ghost copies exchanged once, on the oracle), the same fields."""

    def __init__(self, hip, oracle, geom, periodic, variant):
        configure(hip, oracle, variant)
        self.geom, self.hip, self.oracle = geom, hip, oracle
        self.lo, self.lh = P.new_level(oracle, geom, periodic), P.new_level(hip, geom, periodic)
        for vid, f in P.coefficient_fields(self.lo, 500 + geom[1]).items():
            self.lh.write_all(vid, f)
        self.cells = cell_offsets(self.lh)
        self.held = {}

    @property
    def levels(self):
        return self.lh, self.lo

    def fill(self, name, field):
        self.held[name] = field
        for lv in self.levels:
            lv.write_all(P.IDS[name], field)

    def fill_random(self, names, seed):
        for n, name in enumerate(names):
            self.fill(name, random_field(self.lh, seed + n))

    def fill_box(self, name, box, flat):
        for lv in self.levels:
            lv.write_raw(box, P.IDS[name], flat)

    def destroy(self):
        self.lh.destroy(); self.lo.destroy()


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom, periodic, variant): the levels of one row, made once for the module under the configuration named and left configured so."""
    def get(geom, periodic=False, variant="7pt-cheby-helm", made_for="7pt-cheby-helm"):
        k = (geom, periodic, made_for)
        if k not in _kept:
            _kept[k] = Pair(hip, oracle, geom, periodic, made_for)
        configure(hip, oracle, variant)
        return _kept[k]
    return get


def same_field(got, want, what, nan_matches=False):
    differ = bits(got) != bits(want)
    if nan_matches:
        differ &= ~(np.isnan(got) & np.isnan(want))
    bad = np.argwhere(differ)
    assert bad.size == 0, f"{what}: HIP and oracle differ at (box, raw offset) {bad[:5].tolist()} ..."


def same_passes(R, got, want, took, nan_matches=False):
    """What P.run_passes left on the two sides: which form ran, the three output vectors over whole padded boxes, the operand's interior, the scalars."""
    assert set(got["took"].values()) == {took} and set(want["took"].values()) == {0}, (got["took"], want["took"])
    for key in ("Ap", "x", "r"):
        same_field(got[key], want[key], key, nan_matches)
    same_field(got["p"][:, R.cells], want["p"][:, R.cells], "the interior of p")
    for key in ("pAp", "rmax", "rz", "rz2", "Apz2", "Apz"):
        print(f"{R.geom} {key}: hip {got[key]!r} oracle {want[key]!r}")
        assert P.same_scalar(got[key], want[key]), (key, got[key], want[key])


# live columns of the last block, planes of the last segment, 256 mod side (non-zero: a block starts in the middle of a row)
EDGES = {(1, 1): (1, 1, 0), (1, 4): (16, 4, 0), (1, 12): (144, 12, 4), (1, 20): (144, 4, 16), (3, 12): (144, 12, 4), (2, 24): (64, 8, 16), (1, 40): (64, 8, 16),
         (1, 64): (256, 16, 0), (1, 104): (64, 8, 48), (15, 4): (16, 4, 0), (17, 4): (16, 4, 0), (21, 4): (16, 4, 0)}


@pytest.mark.parametrize("variant", sorted(P.VARIANTS))
@pytest.mark.parametrize("row", P.ROWS, ids=P.row_id)
def test_each_pass_equals_the_oracle(pair_of, row, variant):
    """apply_dot, update (alpha = 0.37), dot, dot2 in an iteration's order on random data in [-1, 1): HIP == oracle for vectors and scalars, dot == the
    restatement, dot2's two values == the two dots."""
    geom, periodic = row
    side = geom[1]
    ncb, nseg, items = P.check_row(geom)
    assert (P.pcg_live_columns(side), side - P.SEGMENT * (nseg - 1), P.COLUMNS % side) == EDGES[geom]
    R = pair_of(geom, periodic, variant)
    a, b = P.VARIANTS[variant]
    R.fill_random(("x", "r", "z", "p"), 7 * geom[0] + side)
    R.fill("Ap", np.full((R.lh.num_boxes, R.lh.volume), np.nan))
    got, want = (P.run_passes(lv, a, b) for lv in R.levels)
    same_passes(R, got, want, took=1)
    assert not np.isnan(got["Ap"][:, R.cells]).any() and np.isnan(np.delete(got["Ap"], R.cells.ravel(), axis=1)).all()
    same_field(got["p"][:, R.cells], R.held["p"][:, R.cells], "p as written")
    assert P.same_scalar(got["rz"], P.dot(R.lo, want["r"], R.held["z"])) and P.same_scalar(got["Apz"], P.dot(R.lo, want["Ap"], R.held["z"]))
    assert P.same_scalar(got["pAp"], P.dot(R.lo, R.held["p"], want["Ap"]))
    assert P.same_scalar(got["rz2"], got["rz"]) and P.same_scalar(got["Apz2"], got["Apz"])
    assert len({got["pAp"], got["rz"], got["Apz"], 0.0}) == 4
    x, r, rmax = P.update(R.lo, R.held["x"], R.held["r"], R.held["p"], want["Ap"], P.ALPHA_CG)
    same_field(got["x"], x, "x against the restatement"); same_field(got["r"], r, "r against the restatement")
    assert got["rmax"] == rmax


# (geometry, box, k, j, i) of the planted maximum
PLACES = {"last-live-column-of-a-ragged-block": ((1, 20), 0, 17, 19, 19),
          "short-last-segment": ((2, 24), 5, 23, 3, 7),
          "box-of-the-last-live-fold-lane": ((17, 4), 4912, 2, 1, 3)}


@pytest.mark.parametrize("where", sorted(PLACES))
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus", "minus"])
def test_update_rmax_wherever_it_sits(pair_of, where, sign):
    """hpgmg_pcg_update's max |r| with +-1e6 planted in one cell of r (everything else in [-1, 1)), as tests/test_gpu_reductions.py
    test_pcg_update_rmax_wherever_it_sits does on the grids of a Solver."""
    geom, box, k, j, i = PLACES[where]
    side = geom[1]
    ncb, nseg, items = P.check_row(geom)
    chunk, live, last = P.pcg_fold_plan(items)
    if where == "last-live-column-of-a-ragged-block":
        assert (i + side * j) // P.COLUMNS == ncb - 1 > 0 and (i + side * j) % P.COLUMNS == P.pcg_live_columns(side) - 1 < P.COLUMNS - 1
    if where == "short-last-segment":
        assert k // P.SEGMENT == nseg - 1 > 0 and side % P.SEGMENT != 0 and 0 < box < geom[0] ** 3 - 1
    if where == "box-of-the-last-live-fold-lane":
        assert (ncb, nseg) == (1, 1) and box // chunk == live - 1 and last == 1 and chunk > 1
    R = pair_of(geom, False, "7pt-cheby")
    R.fill_random(("x", "r", "z", "p", "Ap"), 31 * side + geom[0])
    r = R.held["r"].copy()
    r[box, R.cells[k, j, i]] = sign * HUGE
    R.fill_box("r", box, r[box])
    out = []
    for lv in R.levels:
        took, rmax = P.call_update(lv, "x", "r", "p", "Ap", 1.0e-3)
        out.append((took, rmax, lv.read_all(P.IDS["x"]), lv.read_all(P.IDS["r"])))
    (took_h, rmax_h, x_h, r_h), (took_o, rmax_o, x_o, r_o) = out
    assert (took_h, took_o) == (1, 0)
    x, rn, rmax = P.update(R.lo, R.held["x"], r, R.held["p"], R.held["Ap"], 1.0e-3)
    far = np.abs(rn[:, R.cells])
    assert np.unravel_index(far.argmax(), far.shape) == (box, k, j, i) and far.max() > 0.9 * HUGE and np.sort(far.ravel())[-2] < 1.1
    assert rmax_h == rmax_o == rmax == far.max(), (rmax_h, rmax_o, rmax)
    same_field(x_h, x_o, "x"); same_field(r_h, r_o, "r")
    same_field(x_h, x, "x against the restatement"); same_field(r_h, rn, "r against the restatement")


def three_sums(lv, a, b):
    """dot, dot2 and apply_dot (into the spare vector) on what the level holds: [(took, value ...) ...]"""
    return [P.call_dot(lv, "r", "z"), P.call_dot2(lv, "r", "Ap", "z"), P.call_apply_dot(lv, "spare", "p", a, b)]


def test_a_small_level_after_a_large_one(pair_of):
    """reduction_scratch keeps the 2 x 9261 workgroup values of dot2 at (21, 4) while (1, 4) folds 1 value and (1, 20) 4 (dot2: 2 x 1, 2 x 4) out of
    the same buffer: the small levels' sums must be the bits the oracle gives, which has no scratch to go stale."""
    a, b = P.VARIANTS["7pt-cheby-helm"]
    big = pair_of((21, 4))
    assert P.check_row((21, 4))[2] == 9261
    big.fill_random(("r", "z", "Ap"), 77)
    small = [pair_of(g) for g in ((1, 4), (1, 20))]
    for R in small:
        assert P.check_row(R.geom)[2] < 9261 // 1024
        R.fill_random(("r", "z", "Ap", "p"), 78 + R.geom[1])
    want = [three_sums(R.lo, a, b) for R in small]
    want_big = P.call_dot2(big.lo, "r", "Ap", "z")
    got_big = P.call_dot2(big.lh, "r", "Ap", "z")
    got = [three_sums(R.lh, a, b) for R in small]
    assert got_big[0] == 1 and want_big[0] == 0 and bits(got_big[1:]).tolist() == bits(want_big[1:]).tolist()
    for R, g, w in zip(small, got, want):
        print(R.geom, g, w)
        assert [c[0] for c in g] == [1, 1, 1] and [c[0] for c in w] == [0, 0, 0]
        assert bits([v for c in g for v in c[1:]]).tolist() == bits([v for c in w for v in c[1:]]).tolist()
        assert all(v != 0.0 for c in w for v in c[1:])
        same_field(R.lh.read_all(P.IDS["spare"])[:, R.cells], R.lo.read_all(P.IDS["spare"])[:, R.cells], "A p")


ZERO_ROWS = [(1, 1), (1, 4), (1, 20), (2, 24), (15, 4), (17, 4)]


@pytest.mark.parametrize("a_value,b_value", [(-0.0, 1.0), (-1e-200, 1e-200)], ids=["minus-zero", "underflow"])
@pytest.mark.parametrize("geom", ZERO_ROWS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_a_sum_of_negative_zeros_is_plus_zero(pair_of, geom, a_value, b_value):
    """"a tree value is never -0.0", which is what lets pcg_fold_body skip `+ 0.0` past n and fold more padding than the header names.
    Every product is -0.0 (or underflows to it): dot, both values of dot2 and apply_dot's sum are +0.0 on HIP, sign bit clear, as on the oracle."""
    a, b = P.VARIANTS["7pt-cheby-helm"]
    R = pair_of(geom)
    ones = np.ones((R.lh.num_boxes, R.lh.volume))
    assert np.signbit(a_value * b_value) and a_value * b_value == 0.0
    for name, value in (("r", a_value), ("p", a_value), ("Ap", a_value), ("z", b_value)):
        R.fill(name, value * ones)
    got, want = (three_sums(lv, a, b) for lv in R.levels)
    assert [c[0] for c in got] == [1, 1, 1] and [c[0] for c in want] == [0, 0, 0]
    values = [v for c in got for v in c[1:]]
    assert len(values) == 4 and bits(values).tolist() == [0, 0, 0, 0] == bits([v for c in want for v in c[1:]]).tolist(), (got, want)


@pytest.mark.parametrize("value", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("geom", [(1, 4), (1, 20), (17, 4)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_one_non_finite_cell_in_the_last_box(pair_of, geom, value):
    """+inf (NaN) in the last cell of the last box of r, z = 1 there: dot and dot2's first value are +inf (NaN) on both sides, dot2's second stays
    finite; update drops a NaN candidate of max |r| on both sides and keeps an inf.  Any NaN matches any NaN; everything else is bitwise."""
    a, b = P.VARIANTS["7pt-cheby-helm"]
    R = pair_of(geom)
    side, last = geom[1], R.lh.num_boxes - 1
    R.fill_random(("x", "r", "z", "p", "Ap"), 13 * side + geom[0])
    cell = R.cells[side - 1, side - 1, side - 1]
    r, z = R.held["r"].copy(), R.held["z"].copy()
    r[last, cell], z[last, cell] = value, 1.0
    R.fill_box("r", last, r[last]); R.fill_box("z", last, z[last])
    sums = [(P.call_dot(lv, "r", "z"), P.call_dot2(lv, "r", "Ap", "z")) for lv in R.levels]
    for (took, rz), (took2, rz2, apz) in sums:
        assert rz == np.inf and rz2 == np.inf if value == np.inf else np.isnan(rz) and np.isnan(rz2)
        assert np.isfinite(apz) and apz != 0.0
    assert (sums[0][0][0], sums[0][1][0], sums[1][0][0], sums[1][1][0]) == (1, 1, 0, 0)
    assert P.same_scalar(sums[0][1][2], sums[1][1][2])
    out = []
    for lv in R.levels:
        took, rmax = P.call_update(lv, "x", "r", "p", "Ap", P.ALPHA_CG)
        out.append((took, rmax, lv.read_all(P.IDS["x"]), lv.read_all(P.IDS["r"])))
    (took_h, rmax_h, x_h, r_h), (took_o, rmax_o, x_o, r_o) = out
    x, rn, rmax = P.update(R.lo, R.held["x"], r, R.held["p"], R.held["Ap"], P.ALPHA_CG)
    assert (took_h, took_o) == (1, 0) and P.same_scalar(rmax_h, rmax_o) and rmax_h == rmax
    assert rmax == np.inf if value == np.inf else 0.0 < rmax < 2.0
    same_field(x_h, x_o, "x"); same_field(r_h, r_o, "r", nan_matches=True); same_field(r_h, rn, "r against the restatement", nan_matches=True)


# ---------------------------------------------------------------------------------------------------------------- the portable forms, as the HIP build runs them
PORTABLE_ROWS = [(3, 12), (1, 20)]


def portable_passes(R, a, b):
    R.fill_random(("x", "r", "z", "p"), 5 * R.geom[0] + R.geom[1])
    R.fill("Ap", np.full((R.lh.num_boxes, R.lh.volume), np.nan))
    got, want = (P.run_passes(lv, a, b) for lv in R.levels)
    same_passes(R, got, want, took=0)
    assert len({got["pAp"], got["rz"], got["Apz"], 0.0}) == 4


@pytest.mark.parametrize("geom", PORTABLE_ROWS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_portable_forms_on_constant_coefficients(pair_of, geom):
    """7ptcc-cheby is not a level the kernels take (PORTABLE(...) in host/plugin_pcg.c): the plugin's operators, then the sums on the host from
    downloaded boxes; every call returns 0 and the oracle's bits."""
    R = pair_of(geom, False, "7ptcc-cheby", made_for="7ptcc-cheby")
    portable_passes(R, 0.0, 0.9)


@pytest.mark.parametrize("geom", PORTABLE_ROWS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_portable_forms_with_ghost_free_mode_off(hip, pair_of, geom):
    R = pair_of(geom)
    hip.lib.hpgmg_set_ghost_free(0)
    try:
        portable_passes(R, *P.VARIANTS["7pt-cheby-helm"])
    finally:
        hip.lib.hpgmg_set_ghost_free(1)


@pytest.mark.parametrize("geom", PORTABLE_ROWS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_portable_forms_on_aliased_ids(pair_of, geom):
    """r_id == p_id (r = r - alpha Ap while x = x + alpha times r's old value, cell by cell) and Ap_id == p_id: ids the kernels refuse, so the
    portable forms run and return 0.  update's bits are held to the oracle and the restatement.  apply_op in place has no bits to hold: a cell reads
    neighbours that another thread may or may not have overwritten, and the CPU oracle does not reproduce its OWN result at (1, 20) (two calls on
    equal levels in one process gave p . Ap 2.7e+247 and 6.2e+200 under OpenMP; the MI355X gave 1.3e+14 where the oracle gave 1.0e+247), so only
    the form that ran is asserted and the two values are printed."""
    a, b = P.VARIANTS["7pt-cheby-helm"]
    R = pair_of(geom)
    R.fill_random(("x", "r", "z", "p", "Ap"), 3 * geom[0] + geom[1])
    out = []
    for lv in R.levels:
        took_u, rmax = P.call_update(lv, "x", "r", "r", "Ap", P.ALPHA_CG)
        x, r = lv.read_all(P.IDS["x"]), lv.read_all(P.IDS["r"])
        took_a, pp = P.call_apply_dot(lv, "p", "p", a, b)
        out.append((took_u, rmax, x, r, took_a, pp, lv.read_all(P.IDS["p"])))
    (tu_h, rmax_h, x_h, r_h, ta_h, pp_h, p_h), (tu_o, rmax_o, x_o, r_o, ta_o, pp_o, p_o) = out
    assert (tu_h, ta_h, tu_o, ta_o) == (0, 0, 0, 0)
    x, r, rmax = P.update(R.lo, R.held["x"], R.held["r"], R.held["r"], R.held["Ap"], P.ALPHA_CG)
    same_field(x_h, x_o, "x"); same_field(r_h, r_o, "r"); same_field(x_h, x, "x against the restatement"); same_field(r_h, r, "r against the restatement")
    assert rmax_h == rmax_o == rmax
    print(f"{geom} apply_dot in place: hip {pp_h!r} oracle {pp_o!r}; cells of A p with other bits: {int((bits(p_h[:, R.cells]) != bits(p_o[:, R.cells])).sum())}")
