"""The lifecycle of the dense-array Solver on the CPU oracle: a solver that is kept alive and given new coefficients, right-hand
sides, boundary data, warm starts and methods computes at every step the bits of a fresh solver that has only seen that step's coefficients.
That makes the oracle playing a whole sequence the reference of the GPU tests (test_gpu_user_lifecycle.py), which compare step by step.
"""
import pytest

from hpgmg_testlib import Backend
from user_lifecycle_lib import (PAIR, SPECS, assert_same, differences, fresh, interleave, march_sequence, refused_then_recovered, run, sequence,
                                shift_before, spec_id)


@pytest.fixture(scope="module")
def lib():
    return Backend.oracle().lib


@pytest.mark.parametrize("spec", SPECS, ids=spec_id)
def test_a_reused_solver_equals_a_fresh_one_at_every_step(lib, spec):
    steps = sequence(lib, spec)
    got = run(lib, spec, steps)
    assert [s[0] for s in steps].count("solve") == 7 and len(got) == 11
    for i, step in enumerate(steps):
        if step[0] != "coef":
            bad = differences(got[i], fresh(lib, spec, steps, i))
            assert not bad, f"step {i + 1} ({step[0]}) differs from a fresh solver in {bad}"
    assert not differences(got[10], got[5]), "the last F-cycle is step 6 again"
    assert differences(got[5], got[1]), "the second coefficients changed nothing"
    if spec[2] == ("neumann",) * 6:
        assert all(got[i]["mean_shift"] != 0.0 for i in (1, 5, 6, 7))      # the singular path was taken


@pytest.mark.parametrize("spec", PAIR, ids=spec_id)
def test_a_solver_that_marches_equals_a_fresh_one_at_every_step(lib, spec):
    """The sequence with time marches (user_lifecycle_lib.march_sequence): solves, apply and flux equal a fresh solver created with the live
    solver's current a; a march step equals a fresh solver that was given the coefficients and replays the march from its last start."""
    steps = march_sequence(spec)
    got = run(lib, spec, steps)
    kinds = [s[0] for s in steps]
    assert len(got) == 20 and kinds.count("start") == 4 and kinds.count("step") == 6
    for i, step in enumerate(steps):
        if step[0] in ("solve", "apply", "flux", "step"):
            bad = differences(got[i], fresh(lib, spec, steps, i))
            assert not bad, f"step {i + 1} ({step[0]}) differs from a fresh solver in {bad}"
        else:
            assert got[i] == {}
    assert [shift_before(spec, steps, i) for i in (2, 3, 8, 11, 15, 19)] == [spec[4], 1000.0, 4000.0, 1000.0, spec[4], 2.5]
    for i in (3, 6, 7, 10, 13, 17):
        assert got[i]["rate"] == abs(got[i]["w"]).max() > 0.0 and got[i]["vcycles"] > 0
    assert differences(got[13], got[10]) and differences(got[19], got[1])


def test_two_live_solvers_interleaved_equal_their_solo_runs(lib):
    sequences = [sequence(lib, spec) for spec in PAIR]
    solo = [run(lib, spec, steps) for spec, steps in zip(PAIR, sequences)]
    both = interleave(lib, PAIR, sequences)
    for spec, got, ref in zip(PAIR, both, solo):
        assert_same(got, ref, spec_id(spec))


def test_a_marching_solver_interleaved_with_another_equals_its_solo_run(lib):
    sequences = [march_sequence(PAIR[0]), sequence(lib, PAIR[1])]
    solo = [run(lib, spec, steps) for spec, steps in zip(PAIR, sequences)]
    for spec, got, ref in zip(PAIR, interleave(lib, PAIR, sequences), solo):
        assert_same(got, ref, spec_id(spec))


def test_a_refused_set_coefficients_is_recovered_from(lib):
    got, ref = refused_then_recovered(lib, SPECS[0])
    assert not differences(got, ref)
