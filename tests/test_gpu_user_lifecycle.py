"""The lifecycle of the dense-array Solver on the MI355X: one HIP solver kept alive through new coefficients, right-hand sides,
boundary data, warm starts, methods and switches computes at every step the bits of the CPU oracle, which test_oracle_user_lifecycle.py holds
to a fresh solver per step.  What lives across calls on the HIP side only, and which test reaches it:

  hipGraph segments (kernels/graph.hip, keyed by host/mg.c seg_reset)     test_graph_segments_*: 32^3 / 48^3, every level <= 64^3 lies in segments
  fp32 coefficient copies (plugin_pairs.c coef32_of)                       test_sweep_pair_level_*: 128^3 in boxes of 64, the smallest sweep-pair level
  packed edge coefficients of the sweep-pair pre-pass (pair.hip EdgePack)  test_packed_edge_coefficients_*: 256^3 in boxes of 128 (two 128-cell i tiles)
  staging buffer, lazy queue, one-shot statics, two live solvers           test_reused_solver_*, test_two_live_solvers_*
  all of these across the first start()'s new storage of the finest level  test_a_marching_solver_*, test_packed_edge_coefficients_across_the_storage_*

Every comparison is bitwise.  The switches are the library's own setters; the fixture puts them back (graphs 0, precision 64, fused sweeps 1).
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_testlib import Backend
from test_gpu_user_problem import DeviceArrays
from user_lifecycle_lib import (MARCH_DT, MARCH_RTOL, MARCH_THETA, PAIR, SPECS, Player, assert_same, coefficients, differences, doubled, interleave,
                                issued_thrice, march_sequence, refused_then_recovered, run, sequence, spec_id)

pytestmark = pytest.mark.gpu

PAIR_LEVEL = (128, 64, "dirichlet", "cheby", 1.0)      # the smallest level on the sweep-pair kernel: rows of 128 cells span two boxes
PACKED = (256, 128, "dirichlet", "cheby", 0.0)         # the smallest with packed edge coefficients: two 128-cell i tiles


@pytest.fixture(scope="module")
def libs():
    hip, oracle = Backend.hip().lib, Backend.oracle().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    K.hpgmg_hip_graph_stats.restype, K.hpgmg_hip_graph_stats.argtypes = None, [ctypes.POINTER(ctypes.c_longlong)]
    hip.hpgmg_set_graphs.argtypes = hip.hpgmg_set_fused_sweeps.argtypes = [ctypes.c_int]
    for lib in (hip, oracle):
        lib.hpgmg_set_smoother_precision.argtypes = [ctypes.c_int]
        lib.hpgmg_fp32_pair_smooths.restype = ctypes.c_longlong
    return hip, oracle, K


class Switches:
    def __init__(self, hip, oracle, K):
        self.hip, self.oracle, self.K = hip, oracle, K

    def graphs(self, on):
        self.hip.hpgmg_set_graphs(on)

    def fused_sweeps(self, on):
        self.hip.hpgmg_set_fused_sweeps(on)

    def precision(self, bits):
        for lib in (self.hip, self.oracle):
            lib.hpgmg_set_smoother_precision(bits)

    def graph_stats(self):
        """eager, captured, replayed segments so far"""
        out = (ctypes.c_longlong * 3)()
        self.K.hpgmg_hip_graph_stats(out)
        return list(out)

    def pair_launches(self):
        out = (ctypes.c_longlong * 2)()
        self.K.hpgmg_hip_pair_launch_counts(out)
        return out[0]


@pytest.fixture
def switches(libs):
    sw = Switches(*libs)
    try:
        yield sw
    finally:
        sw.graphs(0)
        sw.precision(64)
        sw.fused_sweeps(1)


@pytest.fixture
def device(libs):
    made = []

    def make():
        made.append(DeviceArrays(libs[2]))
        return made[-1]
    try:
        yield make
    finally:
        for D in made:
            D.free()


def _entry(k, device):
    """host and device entries in turn"""
    return ("device", device()) if k & 1 else ("host", None)


# ---------------------------------------------------------------- reuse = oracle
@pytest.mark.parametrize("k", range(len(SPECS)), ids=[spec_id(s) for s in SPECS])
def test_reused_solver_equals_the_oracle_at_every_step(libs, switches, device, k):
    hip, oracle, _ = libs
    spec, steps = SPECS[k], sequence(oracle, SPECS[k])
    assert_same(run(hip, spec, steps, *_entry(k, device)), run(oracle, spec, steps), spec_id(spec))


# ---------------------------------------------------------------- hipGraph segments under the user API
def _tripled(steps):
    """(steps with every solve issued three times in a row, for each the index of the step it repeats)"""
    out, of = [], []
    for i, step in enumerate(steps):
        for _ in range(3 if step[0] == "solve" else 1):
            out.append(step)
            of.append(i)
    return out, of


@pytest.mark.parametrize("k", range(3), ids=[spec_id(s) for s in SPECS[:3]])
def test_graph_segments_replay_the_oracles_bits_through_the_lifecycle(libs, switches, device, k):
    """Every solve eager, captured and replayed: all three are the oracle's one solve.  After new coefficients, other boundary data or another
    method a graph of the earlier state must not be replayed."""
    hip, oracle, _ = libs
    spec, steps = SPECS[k], sequence(oracle, SPECS[k])
    ref = run(oracle, spec, steps)
    thrice, of = _tripled(steps)
    stats = []
    switches.graphs(1)
    got = run(hip, spec, thrice, *_entry(k + 1, device), after=lambda i, step, out: stats.append(switches.graph_stats()))
    assert_same(got, [ref[i] for i in of], spec_id(spec))
    first = of.index(1)                          # the three issues of step 2
    assert stats[first + 1][1] > stats[first][1], "the second issue captured nothing: graphs are off or fell back to eager"
    assert stats[first + 2][2] > stats[first + 1][2], "the third issue replayed nothing"


def test_graph_segments_with_the_same_key_after_new_coefficients(libs, switches):
    """Every beta doubled, a = 0: D^-1 A and so every eigenvalue bound, hence the key, stay the same, and the graphs captured under the old
    coefficients are replayed.  They must read the new ones: u is the oracle's, and exactly half the earlier u."""
    hip, oracle, _ = libs
    spec = (32, 16, "dirichlet", "cheby", 0.0)
    n = spec[0]
    f = np.random.default_rng(31).random((n, n, n)) - 0.3
    c = coefficients(spec, 32)
    solve = ("solve", f, "fmg", {})
    steps = [("coef", c), solve, solve, solve, ("coef", doubled(c)), solve]
    ref = run(oracle, spec, steps)
    stats, eig = [], []
    switches.graphs(1)
    p = Player(hip, spec)
    try:
        got = []
        for step in steps:
            got.append(p.play(step))
            stats.append(switches.graph_stats())
            if step[0] == "coef":
                G = hip.hpgmg_solver_mg(hip.hpgmg_user_solver_of(p.s._ptr))
                eig.append([hip.hpgmg_level_eigenvalue(hip.hpgmg_mg_level(G, l)) for l in range(hip.hpgmg_mg_num_levels(G))])
    finally:
        p.close()
    assert len(eig[0]) >= 3 and eig[0] == eig[1], "the eigenvalue bounds changed: this is not the same-key case"
    assert stats[3][2] > stats[2][2], "the third solve replayed nothing"
    assert stats[5][2] > stats[4][2] and stats[5][1] == stats[4][1], "the solve after set_coefficients did not replay the cached graphs"
    assert_same(got, ref)
    assert np.array_equal(got[5]["u"], 0.5 * got[3]["u"]) and np.abs(got[3]["u"]).max() > 0.0


def test_graph_segments_follow_the_boundary_data_coming_and_going(libs, switches, device):
    """Without boundary data (eager, captured, replayed), then with, then without, then with other data: the F-cycle's hook adds launches to the
    segments, so a solve with data must not replay a graph captured without."""
    hip, oracle, _ = libs
    spec = SPECS[0]
    n = spec[0]
    rng = np.random.default_rng(41)
    f, g1, g2 = rng.random((n, n, n)) - 0.3, rng.random((6, n, n)) * 4.0 - 2.0, rng.random((6, n, n)) - 0.5
    plain, with1, with2 = ("solve", f, "fmg", {}), ("solve", f, "fmg", {"boundary": g1}), ("solve", f, "fmg", {"boundary": g2})
    steps = [("coef", coefficients(spec, 42)), plain, plain, plain, with1, with1, with1, plain, with2]
    stats = []
    switches.graphs(1)
    got = run(hip, spec, steps, "device", device(), after=lambda i, step, out: stats.append(switches.graph_stats()))
    captured, replayed = [st[1] for st in stats], [st[2] for st in stats]
    assert captured[2] > captured[1] and replayed[3] > replayed[2], "without data: the second solve captured or the third replayed nothing"
    assert captured[5] > captured[4] and replayed[6] > replayed[5], "with data: a key of its own, captured and replayed anew"
    assert replayed[7] > replayed[6] and captured[7] == captured[6], "without data again: the first graphs were not replayed"
    assert replayed[8] > replayed[7] and captured[8] == captured[7], "other data: the hook's graphs read it anew, nothing to capture"
    assert_same(got, run(oracle, spec, steps))
    assert differences(got[4], got[1]) and differences(got[8], got[4])


# ---------------------------------------------------------------- the sweep-pair level and its fp32 coefficient copies
def _pair_level_steps():
    spec = PAIR_LEVEL
    n = spec[0]
    f = np.random.default_rng(128).random((n, n, n)) - 0.3
    c1, c2 = coefficients(spec, 129), coefficients(spec, 130)
    fmg = ("solve", f, "fmg", {})
    # the last two steps go back to c1 after fp32 copies of c2 were made: a copy that outlives set_coefficients is read there
    return [("coef", c1), fmg, ("coef", c2), fmg, ("solve", f, "pcg", {"rtol": 1e-8, "max_iter": 2}), fmg, ("coef", c1), fmg]


@pytest.mark.parametrize("bits", [(64, 64, 64, 64, 64), (64, 32, 64, 32, 32)], ids=["fp64", "toggled"])
def test_sweep_pair_level_equals_the_oracle_through_new_coefficients(libs, switches, bits):
    """128^3: the finest level smooths as sweep pairs.  One live solver through new coefficients and pcg's three more vectors; `toggled`: the
    smoother precision changes between its solves, the oracle's fp32 mode with it."""
    hip, oracle, _ = libs
    steps = _pair_level_steps()
    solves = [i for i, s in enumerate(steps) if s[0] == "solve"]
    counts = {hip: {}, oracle: {}}      # per library and solve step: sweep-pair launches (HIP's, so 0 while the oracle runs) and fp32 smooths

    def count(lib):
        return np.array([switches.pair_launches(), lib.hpgmg_fp32_pair_smooths()])

    def around(lib):
        def before(i, step):
            if step[0] == "solve":
                switches.precision(bits[solves.index(i)])
                counts[lib][i] = count(lib)

        def after(i, step, out):
            if step[0] == "solve":
                counts[lib][i] = count(lib) - counts[lib][i]
        return {"before": before, "after": after}

    ref = run(oracle, PAIR_LEVEL, steps, **around(oracle))
    got = run(hip, PAIR_LEVEL, steps, **around(hip))
    switches.precision(64)
    assert_same(got, ref)
    assert not differences(got[7], got[1]) or bits[0] != bits[4]       # the first coefficients again
    for i, b in zip(solves, bits):
        (pairs, fp32_hip), fp32_oracle = counts[hip][i], counts[oracle][i][1]
        assert pairs > 0, f"step {i + 1} launched no sweep pairs"
        assert fp32_hip == fp32_oracle, f"step {i + 1}: {fp32_hip} fp32 smooths on HIP, {fp32_oracle} on the oracle"
        assert (fp32_hip > 0) == (b == 32), f"step {i + 1} at precision {b}: {fp32_hip} fp32 smooths"
        if b == 32 and steps[i][2] == "fmg":
            assert fp32_hip == 2                 # the two smooths of the 128^3 level in one F-cycle
    if 32 in bits:
        assert differences(got[3], run(hip, PAIR_LEVEL, steps[2:4])[1]), "precision 32 changed nothing"


# ---------------------------------------------------------------- packed edge coefficients
@pytest.fixture(scope="module")
def packed(libs):
    """f and two sets of coefficients at 256^3, and u_ref: u of a fresh solver B with the second set, closed again -- made before any test
    here creates a 256^3 solver of its own."""
    hip, _, K = libs
    n = PACKED[0]
    out = {"f": np.random.default_rng(256).random((n, n, n)) - 0.3, "c1": coefficients(PACKED, 257), "c2": coefficients(PACKED, 258)}
    sw = Switches(*libs)
    before = sw.pair_launches()
    out["u_ref"] = run(hip, PACKED, [("coef", out["c2"]), ("solve", out["f"], "fmg", {})])[1]["u"]
    assert sw.pair_launches() > before, "the 256^3 solve launched no sweep pairs"
    out["u_ref"].setflags(write=False)
    return out


def _count_pairs(switches, pairs):
    """before / after of run(): the sweep-pair launches of every step into pairs[i]"""
    def before(i, step):
        pairs[i] = switches.pair_launches()

    def after(i, step, out):
        pairs[i] = switches.pair_launches() - pairs[i]
    return before, after


def test_packed_edge_coefficients_do_not_outlive_their_solver(libs, switches, packed):
    """A solver's packs are keyed on the device address of its boxes.  Solver B (the fixture's) is closed, solver A with other coefficients
    solves where B was and is closed, and B again gives what it gave."""
    hip = libs[0]
    u_ref = packed["u_ref"]
    fmg = ("solve", packed["f"], "fmg", {})
    pairs = {}
    before, after = _count_pairs(switches, pairs)
    got = run(hip, PACKED, [("coef", packed["c1"]), fmg, ("close_reopen",), ("coef", packed["c2"]), fmg], before=before, after=after)
    assert pairs[1] > 0 and pairs[4] > 0, pairs
    assert got[1]["u"].tobytes() != u_ref.tobytes()            # the other coefficients give another u
    assert got[4]["u"].tobytes() == u_ref.tobytes()


def test_packed_edge_coefficients_follow_set_coefficients(libs, switches, packed, device):
    """One live solver: packs made under the first coefficients, then the second set, then pcg's three more vectors per level; at last without
    the fused sweeps, which use neither packs nor pairs -- the path the rest of the suite holds to the oracle."""
    hip = libs[0]
    u_ref = packed["u_ref"]
    fmg = ("solve", packed["f"], "fmg", {})
    steps = [("coef", packed["c1"]), fmg, ("coef", packed["c2"]), fmg, ("solve", packed["f"], "pcg", {"rtol": 1e-8, "max_iter": 1}), fmg, fmg]
    pairs = {}
    count, after = _count_pairs(switches, pairs)

    def before(i, step):
        if i == len(steps) - 1:
            switches.fused_sweeps(0)
        count(i, step)

    got = run(hip, PACKED, steps, "device", device(), before=before, after=after)
    for i in (3, 5, 6):
        assert got[i]["u"].tobytes() == u_ref.tobytes(), f"step {i + 1}"
    assert got[1]["u"].tobytes() != u_ref.tobytes()
    assert all(pairs[i] > 0 for i in (1, 3, 4, 5)) and pairs[6] == 0, pairs


# ---------------------------------------------------------------- two live solvers, and a refused set_coefficients
@pytest.mark.parametrize("graphs", [0, 1])
def test_two_live_solvers_interleaved_equal_the_oracle(libs, switches, device, graphs):
    hip, oracle, _ = libs
    sequences = [sequence(oracle, spec) for spec in PAIR]
    ref = [run(oracle, spec, steps) for spec, steps in zip(PAIR, sequences)]
    switches.graphs(graphs)
    entry = ("device", [device(), device()]) if graphs else ("host", None)
    for spec, got, want in zip(PAIR, interleave(hip, PAIR, sequences, *entry), ref):
        assert_same(got, want, spec_id(spec))


@pytest.mark.parametrize("graphs", [0, 1])
def test_a_refused_set_coefficients_is_recovered_from(libs, switches, graphs):
    hip, oracle, _ = libs
    want = refused_then_recovered(oracle, SPECS[0])[0]
    switches.graphs(graphs)
    got, fresh = refused_then_recovered(hip, SPECS[0])
    assert not differences(got, want) and not differences(fresh, want)


# ---------------------------------------------------------------- time marches in the lifecycle
@pytest.mark.parametrize("graphs", [0, 1])
@pytest.mark.parametrize("k", range(len(PAIR)), ids=[spec_id(s) for s in PAIR])
def test_a_marching_solver_equals_the_oracle_at_every_step(libs, switches, device, k, graphs):
    """user_lifecycle_lib.march_sequence on one live HIP solver.  Its first start() comes after a solve and gives the finest level new storage
    and a new device box table, under everything the solve left: halo images, the Dinv record and, with graphs on, segments captured and
    replayed over the old storage (every solve is issued three times, every march step followed by two more)."""
    hip, oracle, _ = libs
    spec, steps = PAIR[k], march_sequence(PAIR[k])
    if graphs:
        steps, of = issued_thrice(steps)
    stats = [switches.graph_stats()]
    switches.graphs(graphs)
    got = run(hip, spec, steps, *_entry(k + graphs, device), after=lambda i, step, out: stats.append(switches.graph_stats()))
    switches.graphs(0)
    assert_same(got, run(oracle, spec, steps), spec_id(spec))
    first = [s[0] for s in steps].index("start")              # stats[i]: before step i
    if graphs:
        assert stats[first][1] > stats[0][1] and stats[first][2] > stats[0][2], "nothing was captured and replayed before the first start"
        assert stats[-1][2] > stats[first + 1][2], "nothing was replayed after the first start"
    else:
        assert stats[-1][1:] == stats[0][1:]


@pytest.mark.parametrize("graphs", [0, 1])
def test_a_marching_solver_interleaved_with_another_equals_the_oracle(libs, switches, device, graphs):
    """Two live solvers, one of which marches: its new storage and its set_shift rebuilds come between the other's solves."""
    hip, oracle, _ = libs
    sequences = [march_sequence(PAIR[0]), sequence(oracle, PAIR[1])] if graphs == 0 else [sequence(oracle, PAIR[0]), march_sequence(PAIR[1])]
    ref = [run(oracle, spec, steps) for spec, steps in zip(PAIR, sequences)]
    switches.graphs(graphs)
    entry = ("host", None) if graphs else ("device", [device(), device()])
    for spec, got, want in zip(PAIR, interleave(hip, PAIR, sequences, *entry), ref):
        assert_same(got, want, spec_id(spec))


def test_packed_edge_coefficients_across_the_storage_of_a_first_start(libs, switches, packed):
    """Solver A (Helmholtz) makes its packs in a solve, then start() gives its finest level new storage and a new box table, the key of the
    packs; A steps once and is closed.  Solver B (the fixture's) then gives what it gave.  (By reading: if the new table gets the old address the
    entry is found again and set_shift's rebuild re-packs it; if not it is left behind under the old key, where a later table can meet it only
    after its own rebuild_operator has invalidated that key -- stale values are never read, the buffer stays allocated.)"""
    hip = libs[0]
    spec_a = PACKED[:4] + (1.0,)
    n = spec_a[0]
    rng = np.random.default_rng(259)
    u0, f2 = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 4.0 - 2.0
    fmg = ("solve", packed["f"], "fmg", {})
    pairs = {}
    before, after = _count_pairs(switches, pairs)
    a_steps = [("coef", coefficients(spec_a, 257)), fmg, ("start", u0, packed["f"], None, MARCH_DT, MARCH_THETA), ("step", f2, None, None, None, MARCH_RTOL)]
    got_a = run(hip, spec_a, a_steps, before=before, after=after)
    assert pairs[1] > 0 and pairs[3] > 0, pairs
    assert got_a[3]["converged"] and got_a[3]["rate"] == abs(got_a[3]["w"]).max() > 0.0
    got_b = run(hip, PACKED, [("coef", packed["c2"]), fmg], before=before, after=after)
    assert pairs[1] > 0, pairs
    assert got_b[1]["u"].tobytes() == packed["u_ref"].tobytes()
