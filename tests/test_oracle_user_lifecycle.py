"""The lifecycle of the dense-array Solver on the CPU oracle: a solver that is kept alive and given new coefficients, right-hand
sides, boundary data, warm starts and methods computes at every step the bits of a fresh solver that has only seen that step's coefficients.
That makes the oracle playing a whole sequence the reference of the GPU tests (test_gpu_user_lifecycle.py), which compare step by step.
"""
import pytest

from hpgmg_testlib import Backend
from user_lifecycle_lib import PAIR, SPECS, assert_same, differences, fresh, interleave, refused_then_recovered, run, sequence, spec_id

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


def test_two_live_solvers_interleaved_equal_their_solo_runs(lib):
    sequences = [sequence(lib, spec) for spec in PAIR]
    solo = [run(lib, spec, steps) for spec, steps in zip(PAIR, sequences)]
    both = interleave(lib, PAIR, sequences)
    for spec, got, ref in zip(PAIR, both, solo):
        assert_same(got, ref, spec_id(spec))


def test_a_refused_set_coefficients_is_recovered_from(lib):
    got, ref = refused_then_recovered(lib, SPECS[0])
    assert not differences(got, ref)
