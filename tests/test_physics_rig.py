"""The two comparisons of tests/physics_rig.py that came out of test_gpu_parity.py and have no stand-in test in the suites that use them:
each passes on an honest pair and refuses a wrong one.  CPU only: the backend under test is an oracle, altered by the test.  (The other
comparisons of the rig are held to the same by test_each_new_dimension_bites, test_fp32_oracle_in_the_kernels_place_passes,
test_each_varied_field_bites and test_stand_in_of_the_configuration_itself_passes.)"""
import numpy as np
import pytest

from tests import physics_rig as pr


# ------------------------------------------------------------------------------------------------- assert_same_entries
def test_list_comparison_passes_on_itself_and_refuses_altered_lists():
    """The fp64 oracle's lists of the first teacher-forced sub-step of hand_on_box (N = 256, seed 11: the reference the tumbled-box
    tests compute) at the 2e-6 bound of the parity tests."""
    lists = pr.tumbled_teacher_ref("hand_on_box", pr.N)[0]["lists64"]
    for co in lists:
        pr.assert_same_entries(co, co.copy(), atol=2e-6)
    co = next(c for c in lists if (c[:, 8] == 1).any() and (c[:, 8] == 2).any())       # hand / box and box / ground entries
    hand, ground = int(np.nonzero(co[:, 8] == 1)[0][0]), int(np.nonzero(co[:, 8] == 2)[0][0])
    for row, col, value in ((hand, 9, co[hand, 9] + 1),           # one hand entry's capsule id
                            (ground, 8, 0),                       # one entry's type
                            (hand, 1, co[hand, 1] + 1e-5)):       # one point moved by five times the bound
        ch = co.copy()
        ch[row, col] = value
        with pytest.raises(AssertionError):
            pr.assert_same_entries(co, ch, atol=2e-6)
    ch = co.copy()
    ch[ground, 9] += 1                                             # (the capsule id of a box / ground entry is undefined: not compared)
    pr.assert_same_entries(co, ch, atol=2e-6)


# ------------------------------------------------------------------------------------------------- control_steps
class _Second:
    """A second fp32 oracle in the place of the backend under test; subclasses get one thing wrong."""

    def __init__(self, sc, ms):
        from oracle.oracle import Oracle
        self.o = Oracle(sc, ms)

    def __getattr__(self, name):
        return getattr(self.o, name)


class _ActionsOfTheStepBefore(_Second):
    prev = None

    def step(self, a):
        self.prev, a = a, (np.zeros_like(a) if self.prev is None else self.prev)
        return self.o.step(a)


class _OneDoneFlagFlipped(_Second):
    def step(self, a):
        obs, rew, done = self.o.step(a)
        done[3] = not done[3]
        return obs, rew, done


def _control_steps(second):
    """test_gpu_parity.py::test_other_substep_counts_match_oracle's run and bars at n = 64."""
    from oracle.oracle import Oracle
    sc, _, ms = pr.setup("BlindGrasping", 64, **{"env.episodeLength": 8})
    pr.control_steps(Oracle(sc, ms), second(sc, ms), np.random.default_rng(13), 12,
                     reset_atol=2e-4, obs_bar=5e-3, rew_atol=2e-2, rew_rtol=1e-4, q_atol=5e-4)


def test_control_step_loop_passes_on_an_honest_pair():
    _control_steps(_Second)


def test_control_step_loop_refuses_diverging_observations():
    """Stepped with the actions of the step before, the second instance's observations leave the 5e-3 bar (worst 2.0; the rewards stay
    inside theirs): the assertion on the worst observation error, which carries that error, is the one that fails."""
    with pytest.raises(AssertionError) as e:
        _control_steps(_ActionsOfTheStepBefore)
    assert float(str(e.value)) > 5e-3


def test_control_step_loop_refuses_one_flipped_done_flag():
    with pytest.raises(AssertionError) as e:
        _control_steps(_OneDoneFlagFlipped)
    assert str(e.value) == "0"                                     # the done assertion of step 0
