"""The token hand-overs of the step kernels (broadphase verdicts -> box wave, Schur helpers -> wave 0, the clear mask behind the
phase-1 barrier) at the smallest shapes at which they can go wrong (tests/lds_token_cases.py): one workgroup, a workgroup of 63
padded lanes, and workgroups whose verdict changes within one launch.

Each case runs three control steps (step-kernel launches of four sub-steps) against the fp64 and the fp32 CPU oracle: every step
starts from the fp64 oracle's state rounded to float32 on all three, contact counts, box / ground slot corners and valid cache
slots are exact where the oracles agree, states and cached impulses are held to the rig's error rule (tests/physics_rig.py:
C_RULE x the fp32 oracle's own error, plus the floors).  The diagnostic twin of the library, whose token waits are bounded
(-DDEXSIM_DEBUG_SPIN), must run the same cases without a wait running into its bound and end in the product's bits."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lds_token_cases as lc
from tests import physics_rig as pr
from tests.tumbled_states import f32

CASES = list(lc.CASES)


@functools.lru_cache(maxsize=None)
def _ref(case):
    """Per control step: the state it starts from, both oracles' snapshots after it, the envs the oracles alone decide differently in
    any of its sub-steps, and the hand-contact counts of lc.NEAR at the start of every sub-step (fp32 oracle)."""
    from oracle.oracle import Oracle
    n, start = lc.state(case)
    sc, _, ms = pr.setup("BlindGrasping", n)
    o64, o32 = Oracle(sc, ms, f64=True), Oracle(sc, ms)
    subs, recs = int(sc.substeps), []
    for _ in range(lc.STEPS):
        pr.load(o64, start), pr.load(o32, start)
        left, near = np.zeros(n, bool), []
        for sub in range(subs):
            o64.substep(last=sub == subs - 1), o32.substep(last=sub == subs - 1)
            s64, s32 = pr.snap(o64), pr.snap(o32)
            left |= pr.oracles_differ(s64, s32, ms)
            near.append(lc.hand_contacts(o32, [e for e in lc.NEAR if e < n]))
        recs.append(dict(start=start, s64=s64, s32=s32, left=left, near=near))
        start = {k: f32(o64.get(k)) for k in pr.SYNC}
    return recs


# ------------------------------------------------------------------------------------------------- CPU: the cases are what they claim
def test_shapes():
    assert lc.CASES == {"one_wg": 64, "pad": 65, "mixed": 128}
    assert sorted(e // 64 for e in lc.NEAR) == [0, 1]                    # one descending env in each workgroup


def test_the_oracle_alone_goes_from_clear_to_contact_within_the_first_control_step():
    """mixed: in the fp32 oracle the descending envs have no hand contact in the first sub-step of the first control step (they start
    14 mm above first contact) and hand contacts in its last one, and in every sub-step of the steps after; no other env ever has a
    hand contact; and the oracles never disagree about a descending env, so that the comparison below really includes them."""
    recs = _ref("mixed")
    first = recs[0]["near"]
    assert first[0] == [0, 0] and all(c > 0 for c in first[-1]), first
    for rec in recs[1:]:
        assert all(c > 0 for sub in rec["near"] for c in sub), rec["near"]
    others = np.ones(lc.CASES["mixed"], bool)
    others[list(lc.NEAR)] = False
    for rec in recs:
        assert (rec["s32"]["ncontact"][others] <= 4).all()              # box / ground only
        assert not rec["left"][list(lc.NEAR)].any()
    assert lc.Z0 - (-0.240) > 0.012


@pytest.mark.parametrize("case", ["one_wg", "pad"])
def test_the_random_cases_spread_over_the_heights(case):
    """one_wg / pad: hands well above the box and hands within a few centimetres of first contact (q[2] = -0.240 at the rest pose)."""
    n, start = lc.state(case)
    assert start["q"].shape == (26, n)
    assert (start["q"][2] > -0.1).any() and (start["q"][2] < -0.15).any()


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_three_control_steps_against_the_oracles(case):
    recs = _ref(case)
    n = lc.CASES[case]
    sc, _, ms = pr.setup("BlindGrasping", n)
    same = ~pr.left_by_the_references(recs)
    b = pr.hip(sc, ms)
    probe = b.core.set_phase_probe(True) if case == "mixed" else None
    report = {}
    for t, rec in enumerate(recs):
        pr.load(b, rec["start"])
        b.physics_step()
        sh = pr.snap(b)
        if case == "mixed" and t == 0:
            general = probe[:, 2].cpu().numpy()
            print(f"\nsub-steps of the first control step on the general path, per workgroup: {general}")
            assert ((general >= 1) & (general <= 3)).all(), general     # the verdict changed within the launch, in both workgroups
            b.core.set_phase_probe(False)
        same = pr.agree(same, rec["s64"]["ncontact"], rec["s32"]["ncontact"], sh["ncontact"])
        assert (sh["corner"][:, same] == rec["s64"]["corner"][:, same]).all(), "a box / ground slot holds another corner"
        pr.assert_same_slots(sh, rec["s64"], same)
        pr.accumulate_snap(report, rec["s64"], rec["s32"], sh, same, pr.FIELDS)
    if case == "mixed":
        assert same[list(lc.NEAR)].all()
    pr.assert_c_rule(report, f"three control steps, {case}, n = {n}")


@pytest.mark.gpu
def test_the_bounded_twin_hits_no_bound_and_ends_in_the_same_bits():
    from dexrobot_isaac_amd.build import DEBUG_SPIN_LIB
    from tests.lds_token_child import run_case
    assert os.path.exists(DEBUG_SPIN_LIB), "build it with __graft_entry__.build() / build_debug_spin()"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lds_token_child.py")
    out = subprocess.run([sys.executable, child, *CASES], env={**os.environ, "DEXSIM_LIB_PATH": DEBUG_SPIN_LIB}, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    debug = json.loads(out.stdout.strip().splitlines()[-1])
    for case in CASES:
        assert debug[case]["spin_word"] == 0, f"{case}: a token wait ran into its bound, site/seq word {debug[case]['spin_word']:#x}"
        assert debug[case]["digest"] == run_case(case)["digest"], case
