"""The states of tests/test_lds_token_paths.py and of its child process (tests/lds_token_child.py): the smallest shapes at which the
token code of the step kernels (waits, votes, the posts of the Schur helpers) can go wrong.  A plain module like tumbled_states: no
fixtures, no torch.

  one_wg   N = 64: one workgroup;
  pad      N = 65: two workgroups, the second with ONE real lane -- its 63 padded lanes take part in every vote;
           (both: the hands of physics_rig.random_state(near_box=False) -- most of them clear of everything, the regime of the
           headline -- over boxes AT REST on the ground as a reset leaves them.  random_state's own boxes start up to 0.5 mm inside
           the ground or up to 4.5 mm above it, spinning: the rig steps that class one teacher-forced sub-step at a time, n = 512.
           Free-running over the four sub-steps of a launch a box that lands on an edge amplifies roundoff: with those boxes "pad"
           missed the rule in ONE entry, box_ang of env 0 after the second step, 6.39e-5 against 3 x 2.07e-5 + 1e-6 -- in the
           same bits with the library as it was before the token waits changed.  That is the box solver's accuracy on a tumbling
           box, which tests/test_tumbled_box.py holds on its own samples; it is not what these shapes are here for.)
  mixed    N = 128: one env per workgroup (NEAR) comes down on its box so fast that, within the first control step, the
           workgroup's broadphase verdict is "clear" in the first sub-steps and "not clear" in the last: the box wave drops its
           speculative sweeps half-way and both forms of the Schur phase (split with helper tokens / unsplit) run in ONE launch.
           Every other env stays far above its box.

A control step here is the step kernel's launch of one physics step (sim.substeps = 4 sub-step bodies, DexSimCore.physics_step)."""
import numpy as np

from tests import physics_rig as pr

STEPS = 3
CASES = {"one_wg": 64, "pad": 65, "mixed": 128}
NEAR = (5, 64 + 41)            # the descending envs of "mixed", one per workgroup
# "mixed": the hand at rest pose touches the box at q[2] = -0.240 (first contact of the fp32 oracle, box at rest on the ground).  It
# starts Z0 - (-0.240) = 14 mm above that and falls at V0: 7.5 mm per sub-step (h = 2.5 ms), so sub-step 1 starts 14 mm and sub-step 2
# 6.5 mm away -- beyond what the per-capsule bounds add to a capsule's own extent -- and sub-steps 3 or 4 start in contact.
Z0, V0, Z_TARGET = -0.226, -3.0, -0.30


def box_at_rest(n):
    z = np.zeros((1, n))
    return dict(box_pos=np.concatenate([z, z, z + 0.0255]), box_quat=np.concatenate([z, z, z, z + 1.0]), box_lin=np.zeros((3, n)),
                box_ang=np.zeros((3, n)))


def state(case):
    """(n, start state) of a case, deterministic."""
    n = CASES[case]
    _, model, _ = pr.setup("BlindGrasping", n)
    rng = np.random.default_rng({"one_wg": 64, "pad": 65, "mixed": 128}[case])
    if case != "mixed":
        return n, {**pr.random_state(rng, model, n, near_box=False), **box_at_rest(n)}
    q = np.zeros((26, n))
    q[:2] = rng.uniform(-0.1, 0.1, (2, n))
    q[2] = rng.uniform(0.0, 0.2, n)
    q[6:] = rng.uniform(0.0, 0.3, (20, n))
    qd = rng.normal(0, 0.3, (26, n))
    tg = q + rng.normal(0, 0.05, (26, n))
    for e in NEAR:
        q[:, e], qd[:, e], tg[:, e] = 0.0, 0.0, 0.0
        q[2, e], qd[2, e], tg[2, e] = Z0, V0, Z_TARGET
    return n, dict(q=q, qd=qd, targets=tg, **box_at_rest(n))


def hand_contacts(b, envs):
    """How many entries of the listed envs' contact lists are hand contacts (types 0 and 1)."""
    return [int((b.contacts(e)[:, 8] != 2).sum()) for e in envs]
