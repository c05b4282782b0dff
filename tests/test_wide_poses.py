"""The step kernels' hand dynamics over the WHOLE joint range, at speed and at the joint stops (tests/wide_states.py), against the fp64
and fp32 oracles: the method of tests/test_tumbled_box.py (teacher-forced sub-steps, bounds from the fp32 oracle's own error) along the
hand's state instead of the box's.  Contact-free on purpose: the hand is >= 0.3 m above box and ground, so there is no contact-set
bifurcation and the only discontinuity is the joint-limit clamp behind the integration, which is handled explicitly (below).

Every other GPU physics test draws finger joints from [0, 0.5] rad, base rotations from +-0.3 rad and speeds from N(0, 0.3), clipped away
from every limit.  Three parts of the step kernels therefore run without anything looking at their result:
  the velocity terms of the bias force   removing them moves qd after one sub-step by 4.4 bounds on that sample, by hundreds here;
  the quadrant logic of sincos_joint     no half-angle leaves quadrant 0 there (that needs |q| > pi / 2); about half the base rotations here;
  the joint-limit clamp                  no teacher-forced state reaches a stop there; a thousand joint-sub-steps end clamped here.

N = 256 envs, seed 11 (four workgroups), and the first 200 envs (last workgroup padded).  Bounds: none of this file's own.  States and
published quantities: the error against fp64 at the 99.9th percentile and at the maximum is at most c = 3 x the fp32 oracle's own error
on the same entries, plus the floors 1e-7 and 1e-6 (tests/physics_rig.py::accumulate / assert_c_rule).  Contact counts exact.

The clamp.  A third fp64 oracle instance runs a model whose limits are widened by +-10 and is re-synchronised from the clamped fp64
oracle before every sub-step; its unclamped q classifies every joint-sub-step: beyond a stop by more than 1e-5 rad -- clamped, inside by
more than 1e-5 rad -- free, otherwise ambiguous (roundoff decides).  On clamped joints q must equal the float32 limit and qd must be 0,
exactly.  Ambiguous joints are left out of the qd comparison of that sub-step (q is continuous across the clamp and stays in); at most
LEFT_OUT = 2 % of the envs may hold one (the sample holds none).

The CPU tests show that what the GPU tests rely on holds for the reference alone -- the sample covers the cases, no env has a hand
contact, the clamp is the stated rule to the bit, the oracle's sub-step is the textbook implicit-PD step on M and b -- and that every new
dimension BITES: an fp32 stand-in with the velocity terms dropped, a limit moved, a clamp that does not stop the joint or a wrong
quadrant is refused by the very functions the GPU tests call, while the fp32 oracle itself passes.  Measured figures: DESIGN.md, section 5.
"""
import copy
import functools

import numpy as np
import pytest

from tests import physics_rig as pr
from tests import wide_states as ws
from tests.tumbled_states import f32

N, SEED, PADDED = pr.N, pr.SEED, 200
KINDS = ("free", "stops")
WIDEN = 10.0                            # the third instance's limits: lo - 10, hi + 10
AMBIGUOUS = 1e-5                        # rad: an unclamped q this close to a stop is decided by roundoff
THUMB = 6                               # the first thumb joint, range [0, 1.7]: the only finger joint that can pass pi / 2
LOWERED = 6 + 4 * 1 + 1                 # stand-in (b): this joint's hi lowered by 1e-3
HAND_FIELDS = ("q", "qd")
PUBLISHED = ("site_pose", "hand_vel")


# ------------------------------------------------------------------------------------------------- configurations and states
def _setup(task, n, name=None):
    """(sc, model, ms) for n envs; name: a model of pr.MODELS that lacks the folded structure."""
    return pr.setup(task, n, model=name)


def _variant(task, n, name=None, widen=0.0, lower=None):
    """(sc, ms) of the same configuration with every limit widened by +-widen and / or joint `lower`'s hi lowered by 1e-3."""
    sc, model, _ = _setup(task, n, name)
    m = copy.deepcopy(model)
    m.lo, m.hi = m.lo - widen, m.hi + widen
    if lower is not None:
        m.hi[lower] -= 1e-3
    return sc, m.to_struct()


def _state(kind, n, task="BlindGrasping", name=None):
    """The first n envs of the N-env sample drawn for the configuration (no box fields for BaseTask)."""
    sc, model, _ = _setup(task, N, name)
    st = ws.sample(kind, N, SEED, config=(sc, model))
    return {k: v[:, :n].copy() for k, v in st.items() if task == "BlindGrasping" or not k.startswith("box")}


def _sync(task):
    return pr.SYNC if task == "BlindGrasping" else HAND_FIELDS


def _snap(b, task):
    if task == "BlindGrasping":
        return pr.snap(b)
    s = {f: b.get(f) for f in HAND_FIELDS}
    s["ncontact"] = b.get("ncontact")[0].astype(int)
    return s


def _classify(qw, lo, hi):
    """Per joint and env from the widened instance's unclamped q: clamped at lo, clamped at hi, ambiguous."""
    over_lo, over_hi = lo[:, None] - qw, qw - hi[:, None]
    amb = (np.abs(over_lo) <= AMBIGUOUS) | (np.abs(over_hi) <= AMBIGUOUS)
    return (over_lo > AMBIGUOUS), (over_hi > AMBIGUOUS), amb


# ------------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=None)
def _teacher_ref(kind, n, task="BlindGrasping", name=None):
    """pr.teacher_ref with the widened instance next to the two oracles: three teacher-forced sub-steps, after each q, qd and the box
    state of all three are put to the (clamped) fp64 oracle's values rounded to float32.  Per sub-step: the float32 state it started
    from, both snapshots, both contact lists, the widened instance's unclamped q and qd and the classification they give; with the
    last one, what both oracles publish from their own final state."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup(task, n, name)
    lo, hi = ws.limits(ms)
    o64, o32, w64 = Oracle(sc, ms, f64=True), Oracle(sc, ms), Oracle(*_variant(task, n, name, widen=WIDEN), f64=True)
    start = _state(kind, n, task, name)
    out = []
    for sub in range(3):
        for o in (o64, o32, w64):
            pr.load(o, start)
            o.substep(last=True)
        rec = dict(start=start, s64=_snap(o64, task), s32=_snap(o32, task), lists64=pr.lists(o64, n), lists32=pr.lists(o32, n),
                   qw=w64.get("q"), qdw=w64.get("qd"))
        rec["at_lo"], rec["at_hi"], rec["amb"] = _classify(rec["qw"], lo, hi)
        out.append(rec)
        start = dict(start, **{k: f32(o64.get(k)) for k in _sync(task)})
    o64.publish(), o32.publish()
    out[-1]["pub64"], out[-1]["pub32"] = {f: o64.get(f) for f in PUBLISHED}, {f: o32.get(f) for f in PUBLISHED}
    return out


@functools.lru_cache(maxsize=None)
def _free_ref(n):
    """The `stops` sample free-running for one physics step (sim.substeps sub-steps) on both oracles; the widened instance takes the
    fp64 oracle's state before every sub-step, an env with an ambiguous joint stays out from then on."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup("BlindGrasping", n)
    lo, hi = ws.limits(ms)
    o64, o32, w64 = Oracle(sc, ms, f64=True), Oracle(sc, ms), Oracle(*_variant("BlindGrasping", n, widen=WIDEN), f64=True)
    st = _state("stops", n)
    for o in (o64, o32, w64):
        pr.load(o, st)
    left, subs = np.zeros(n, bool), int(sc.substeps)
    for sub in range(subs):
        pr.load(w64, {k: o64.get(k) for k in pr.SYNC})
        for o in (o64, o32, w64):
            o.substep(last=sub == subs - 1)
        at_lo, at_hi, amb = _classify(w64.get("q"), lo, hi)
        left |= amb.any(0)
    return dict(s64=pr.snap(o64), s32=pr.snap(o32), left=left, at_lo=at_lo, at_hi=at_hi)


# ------------------------------------------------------------------------------------------------- the comparisons (GPU tests and stand-ins)
def _accumulate_rec(report, s64, s32, sh, amb, left):
    """pr.accumulate per field over the envs not in `left`; qd without the ambiguous joints."""
    keep = ~left
    for f in s64:
        if f in pr.SNAP_EXTRAS:
            continue
        mask = np.broadcast_to(keep, s64[f].shape)
        pr.accumulate(report, f, s64[f], s32[f], sh[f], mask & ~amb if f == "qd" else mask)
    if "lam" in s64:
        ok = (s64["corner"] >= 0) & (s64["corner"] == s32["corner"]) & (s64["corner"] == sh["corner"]) & keep
        pr.accumulate(report, "wlam 80-83", s64["lam"], s32["lam"], sh["lam"], np.repeat(ok, 3, axis=0))


def _assert_no_hand_contact(sh, rec, task):
    for s in (rec["s64"], rec["s32"]):
        assert (sh["ncontact"] == s["ncontact"]).all(), f"contact count differs in {(sh['ncontact'] != s['ncontact']).sum()} envs"
    assert sh["ncontact"].max() <= 4                                   # box / ground only: the hand-clear early box solve really ran
    if task == "BlindGrasping":
        assert (sh["corner"] == rec["s64"]["corner"]).all(), "a box / ground slot holds another corner"


def _assert_on_the_stops(sh, at_lo, at_hi, lo, hi, keep=None):
    """On the joints the widened instance puts beyond a stop: q is the float32 limit and qd is 0, exactly."""
    keep = np.ones(at_lo.shape[1], bool) if keep is None else keep
    for at, lim in ((at_lo, lo), (at_hi, hi)):
        at = at & keep
        q, want = sh["q"][at], np.broadcast_to(lim[:, None], at.shape)[at]
        assert (q == want).all(), f"{(q != want).sum()} of {at.sum()} clamped joints are not on the limit (worst {np.abs(q - want).max():.3g})"
        assert (sh["qd"][at] == 0).all(), f"{(sh['qd'][at] != 0).sum()} of {at.sum()} clamped joints still move (worst {np.abs(sh['qd'][at]).max():.3g})"


def _run_teacher(make, kind, n, task="BlindGrasping", name=None, exact=True):
    """The three teacher-forced sub-steps on the backend that make() returns: (backend, report).  exact = False skips the exact
    assertions (contact counts, joints on their stops), for the margins of the stand-ins."""
    recs = _teacher_ref(kind, n, task, name)
    lo, hi = ws.limits(_setup(task, n, name)[2])
    b, report, none_left = make(), {}, np.zeros(n, bool)
    for rec in recs:
        pr.load(b, rec["start"])
        b.substep(last=True)
        sh = _snap(b, task)
        assert rec["amb"].any(0).mean() <= pr.LEFT_OUT, f"{rec['amb'].any(0).sum()} of {n} envs hold an ambiguous joint"
        if exact:
            _assert_no_hand_contact(sh, rec, task)
            _assert_on_the_stops(sh, rec["at_lo"], rec["at_hi"], lo, hi)
        _accumulate_rec(report, rec["s64"], rec["s32"], sh, rec["amb"], none_left)
    return b, report


def _label(what, kind, n, task, name):
    return f"{what}, {kind}, {task}{'' if name is None else ', model ' + name}, n = {n}"


def _check_teacher(make, kind, n, task="BlindGrasping", name=None):
    """Item 5: states after each of three teacher-forced sub-steps by the c rule, contact counts and clamped joints exact."""
    _, report = _run_teacher(make, kind, n, task, name)
    pr.assert_c_rule(report, _label("teacher-forced", kind, n, task, name))
    assert ("wlam 80-83" in report) == (task == "BlindGrasping")
    return report


def _body_states(hk, q, qd, dtype, envs):
    """Origins (k, 37, 3) and twists (k, 37, 6) of the hand bodies from tests/kindyn_ref.HandKin, evaluated in `dtype`."""
    pos, twist = [], []
    for e in envs:
        x, v = q[:, e].astype(dtype), qd[:, e].astype(dtype)
        pos.append(hk.body_frames(x, dtype)[0])
        twist.append(hk.jacobian(x, dtype) @ v)
    return np.stack(pos).astype(np.float64), np.stack(twist).astype(np.float64)


def _published_report(make, kind, n, task="BlindGrasping", name=None):
    b, _ = _run_teacher(make, kind, n, task, name, exact=False)
    rec = _teacher_ref(kind, n, task, name)[-1]
    b.publish()
    report, every = {}, np.ones(n, bool)
    for f in PUBLISHED:
        pr.accumulate(report, f, rec["pub64"][f], rec["pub32"][f], b.get(f), np.broadcast_to(every, rec["pub64"][f].shape))
    core = getattr(b, "core", None)
    if core is not None:
        import torch
        from tests import kindyn_ref as kr
        hk, envs = kr.HandKin(_setup(task, n, name)[2]), np.arange(0, n, 4)
        core.refresh_body_states()
        torch.cuda.synchronize()
        rbs = core.rigid_body_states[:, :kr.NB].cpu().numpy().astype(np.float64)[envs]
        p64, t64 = _body_states(hk, rec["s64"]["q"], rec["s64"]["qd"], np.float64, envs)
        p32, t32 = _body_states(hk, rec["s32"]["q"], rec["s32"]["qd"], np.float32, envs)
        pr.accumulate(report, "body pos", p64, p32, rbs[:, :, 0:3], np.ones(p64.shape, bool))
        pr.accumulate(report, "body twist", t64, t32, rbs[:, :, 7:13], np.ones(t64.shape, bool))
    return report


def _check_published(make, kind, n, task="BlindGrasping", name=None):
    """Item 6: after the last teacher-forced sub-step every side publishes from its own state: site_pose and hand_vel by the c rule
    against the oracles; on a backend with rigid_body_states also the origins and twists of the 37 hand bodies of every fourth env,
    against tests/kindyn_ref.HandKin in float64 on the fp64 oracle's final state and in float32 on the fp32 oracle's."""
    report = _published_report(make, kind, n, task, name)
    pr.assert_c_rule(report, _label("published", kind, n, task, name))
    return report


def _check_physics_step(make, n, exact=True):
    """Item 7: one free-running physics step from the `stops` sample against both oracles: contact counts exact, states by the c
    rule over the envs that held no ambiguous joint in any sub-step, joints clamped in the last sub-step on their stops."""
    ref = _free_ref(n)
    lo, hi = ws.limits(_setup("BlindGrasping", n)[2])
    assert ref["left"].mean() <= pr.LEFT_OUT, f"{ref['left'].sum()} of {n} envs left out"
    b = make()
    pr.load(b, _state("stops", n))
    b.physics_step()
    sh = pr.snap(b)
    if exact:
        _assert_no_hand_contact(sh, ref, "BlindGrasping")
        _assert_on_the_stops(sh, ref["at_lo"], ref["at_hi"], lo, hi, ~ref["left"])
    report = {}
    _accumulate_rec(report, ref["s64"], ref["s32"], sh, np.zeros((26, n), bool), ref["left"])
    pr.assert_c_rule(report, f"one physics step, stops, n = {n}")
    return report


# ------------------------------------------------------------------------------------------------- CPU: the sample
def _quadrant(q):
    """sincos_joint's k for the joint angle q: the quadrant of the half-angle."""
    return np.rint(0.5 * q * 2.0 / np.pi)


def test_sample_covers_the_cases():
    """What the sample holds and what the fp64 oracle makes of it; every threshold is half of the count observed at N = 256, seed 11."""
    from oracle.oracle import Oracle
    free, stops = _teacher_ref("free", N), _teacher_ref("stops", N)
    q = free[0]["start"]["q"]
    base_k, thumb_k = int((_quadrant(q[3:6]) != 0).sum()), int((_quadrant(q[THUMB]) != 0).sum())
    clamped = [int((r["at_lo"] | r["at_hi"]).sum()) for r in stops]
    at_lo, at_hi = [int(r["at_lo"].sum()) for r in stops], [int(r["at_hi"].sum()) for r in stops]
    free_clamped = [int((r["at_lo"] | r["at_hi"]).sum()) for r in free]
    speed = np.abs(free[0]["start"]["qd"])
    print(f"\nbase rotations outside quadrant 0: {base_k} of {q[3:6].size}; first thumb joints: {thumb_k} of {N}; joint-sub-steps that end "
          f"clamped, stops: {clamped} (lo {at_lo}, hi {at_hi}), free: {free_clamped}; |qd| median fingers {np.median(speed[6:]):.2f}, "
          f"base rotations {np.median(speed[3:6]):.2f}")
    # observed: 377 of 768 base rotations, 18 of 256 first thumb joints
    assert base_k >= 188 and thumb_k >= 9
    # observed: 1034 / 1039 / 1043 joint-sub-steps end clamped on `stops` (at lo 497 / 500 / 502, at hi 537 / 539 / 541); 12 / 20 / 29 on `free`
    assert all(c >= 517 for c in clamped) and all(c >= 248 for c in at_lo) and all(c >= 268 for c in at_hi)
    for kind, recs in (("free", free), ("stops", stops)):
        for rec in recs:
            on = rec["at_lo"] | rec["at_hi"]
            assert (rec["s64"]["qd"][on] == 0).all(), kind                       # every clamped joint stands still in the fp64 oracle
            for s, lists in ((rec["s64"], rec["lists64"]), (rec["s32"], rec["lists32"])):
                assert s["ncontact"].max() <= 4 and all((c[:, 8] == 2).all() for c in lists), kind     # box / ground only, no env left out
    # the free run takes the same sub-steps as physics_step, and lists no hand contact either
    sc, _, ms = _setup("BlindGrasping", N)
    o = Oracle(sc, ms, f64=True)
    pr.load(o, _state("stops", N))
    o.physics_step()
    ref = _free_ref(N)
    assert all(np.array_equal(o.get(f), ref["s64"][f]) for f in pr.FIELDS) and ref["s64"]["ncontact"].max() <= 4
    assert all((c[:, 8] == 2).all() for c in pr.lists(o, N))


def test_sample_covers_the_cases_generic_model():
    """The conditions the GPU tests on the `generic` model (tests/generic_model.py) rely on, from the references alone: the sample
    drawn for its limits covers the quadrants and the stops as the default one does, no env lists a hand contact (the hand_reach of
    this model under its turned spawn frame included), every clamped joint stands still, at most LEFT_OUT of the envs hold a joint
    that roundoff decides, and the two oracles alone decide at most LEFT_OUT of the envs differently (physics_rig.oracles_differ)."""
    name = "generic"
    free, stops = _teacher_ref("free", N, name=name), _teacher_ref("stops", N, name=name)
    ms = _setup("BlindGrasping", N, name)[2]
    q = free[0]["start"]["q"]
    base_k, thumb_k = int((_quadrant(q[3:6]) != 0).sum()), int((_quadrant(q[THUMB]) != 0).sum())
    clamped = [int((r["at_lo"] | r["at_hi"]).sum()) for r in stops]
    at_lo, at_hi = [int(r["at_lo"].sum()) for r in stops], [int(r["at_hi"].sum()) for r in stops]
    amb = [float(r["amb"].any(0).mean()) for recs in (free, stops) for r in recs]
    left = [float(pr.oracles_differ(r["s64"], r["s32"], ms).mean()) for recs in (free, stops) for r in recs]
    print(f"\ngeneric model: base rotations outside quadrant 0: {base_k} of {q[3:6].size}; first thumb joints: {thumb_k} of {N}; joint-sub-steps "
          f"that end clamped, stops: {clamped} (lo {at_lo}, hi {at_hi}); share of envs with an ambiguous joint per sub-step {amb}; "
          f"share the oracles decide differently {left}")
    assert base_k >= 188 and thumb_k >= 9                                       # the thresholds of test_sample_covers_the_cases
    assert all(c >= 517 for c in clamped) and all(c >= 248 for c in at_lo) and all(c >= 268 for c in at_hi)
    assert max(amb) <= pr.LEFT_OUT and max(left) <= pr.LEFT_OUT
    for kind, recs in (("free", free), ("stops", stops)):
        pr.left_by_the_references([dict(left=pr.oracles_differ(r["s64"], r["s32"], ms)) for r in recs])
        for rec in recs:
            on = rec["at_lo"] | rec["at_hi"]
            assert (rec["s64"]["qd"][on] == 0).all(), kind
            for s, lists in ((rec["s64"], rec["lists64"]), (rec["s32"], rec["lists32"])):
                assert s["ncontact"].max() <= 4 and all((c[:, 8] == 2).all() for c in lists), kind


@pytest.mark.parametrize("task,name", [("BlindGrasping", None), ("BaseTask", None), ("BlindGrasping", "all"), ("BlindGrasping", "generic")],
                         ids=["default", "basetask", "model-all", "generic"])
def test_joints_decided_by_roundoff_and_the_clamp_rule(task, name):
    """Item 2.  No env of either kind holds an ambiguous joint in any sub-step (the GPU tests allow 2 %), in the free run neither; and
    the oracle's clamp is the stated rule, to the bit: its q is clip(q_unclamped, lo, hi) and its qd the one-sided max / min of the
    unclamped qd, with lo / hi the float32 numbers of the model struct (with the Python model's doubles q is off by 4.8e-8)."""
    _, model, ms = _setup(task, N, name)
    lo, hi = ws.limits(ms)
    worst = 0.0
    for kind in KINDS:
        for sub, rec in enumerate(_teacher_ref(kind, N, task, name)):
            share = rec["amb"].any(0).mean()
            assert share == 0.0, (kind, sub, share)                             # the condition of the issue is <= LEFT_OUT; the draw gives 0
            qw, qdw = rec["qw"], rec["qdw"]
            q = np.clip(qw, lo[:, None], hi[:, None])
            qd = np.where(qw < lo[:, None], np.maximum(qdw, 0), np.where(qw > hi[:, None], np.minimum(qdw, 0), qdw))
            assert np.array_equal(rec["s64"]["q"], q) and np.array_equal(rec["s64"]["qd"], qd), (kind, sub)
            worst = max(worst, np.abs(rec["s64"]["q"] - np.clip(qw, model.lo[:, None], model.hi[:, None])).max())
    print(f"\n{task}, {name}: clamp against the struct's float32 limits: exact; against the Python model's doubles: {worst:.2e}")
    assert worst < 1e-7
    assert (worst > 0) == bool((f32(model.lo) != model.lo).any() or (f32(model.hi) != model.hi).any())   # (the generic model's limits are float32 numbers)
    if task == "BlindGrasping" and name is None:
        assert _free_ref(N)["left"].sum() == 0


def _implicit_pd_step(orc, ms, h, st, dtype=np.float64, velocity_terms=True):
    """The sub-step of a contact-free hand written out in numpy, unclamped: M, b from Oracle.mass_matrix, Mhat = M + diag(armature +
    h (k_d + h k_p)), tau = k_p (q* - q) - (k_d + h k_p) qd - b, qd+ = qd + Mhat^-1 h tau, q+ = q + h qd+.  Evaluated in `dtype`;
    velocity_terms = False takes b(q, 0) in place of b(q, qd)."""
    arm, kp, kd = (np.array(np.ctypeslib.as_array(getattr(ms, k)), dtype=dtype) for k in ("armature", "kp", "kd"))
    h = dtype(h)
    q, qd, tg = (st[k].astype(dtype) for k in ("q", "qd", "targets"))
    qn, vn = np.zeros_like(q), np.zeros_like(q)
    for e in range(q.shape[1]):
        M, b = orc.mass_matrix(q[:, e], qd[:, e] if velocity_terms else np.zeros(26))
        Mh = M.astype(dtype) + np.diag(arm + h * (kd + h * kp))
        tau = kp * (tg[:, e] - q[:, e]) - (kd + h * kp) * qd[:, e] - b.astype(dtype)
        vn[:, e] = qd[:, e] + np.linalg.solve(Mh, h * tau)
        qn[:, e] = q[:, e] + h * vn[:, e]
    assert qn.dtype == dtype
    return qn.astype(np.float64), vn.astype(np.float64)


def test_substep_is_the_implicit_pd_step_on_mass_matrix_and_bias():
    """Item 3.  An integrator the oracle's sub-step does not share (numpy's LU solve in place of its Cholesky, one formula in place of
    its loops) against the widened fp64 instance, every env, every sub-step, both kinds: measured 4.4e-16 on q and 9.8e-15 on qd; the
    bound 1e-10 is far above fp64 roundoff and far below any fp32 bound used here.  tests/test_oracle_physics.py pins M and b
    themselves at rows of this sample."""
    from oracle.oracle import Oracle
    sc, _, ms = _setup("BlindGrasping", N)
    o, h = Oracle(sc, ms, f64=True), float(sc.dt) / int(sc.substeps)
    worst = [0.0, 0.0]
    for kind in KINDS:
        for rec in _teacher_ref(kind, N):
            q, qd = _implicit_pd_step(o, ms, h, rec["start"])
            worst = [max(worst[0], np.abs(q - rec["qw"]).max()), max(worst[1], np.abs(qd - rec["qdw"]).max())]
    print(f"\nnumpy integrator against the widened fp64 oracle: q {worst[0]:.2e}, qd {worst[1]:.2e}")
    assert worst[0] <= 1e-10 and worst[1] <= 1e-10


# ------------------------------------------------------------------------------------------------- CPU: every new dimension bites
class _StandIn:
    """An fp32 oracle in the kernels' place, with one thing wrong (subclasses)."""

    def __init__(self, sc, ms):
        from oracle.oracle import Oracle
        self.o = Oracle(sc, ms)

    def set(self, k, v):
        self.o.set(k, v)

    def get(self, k):
        return self.o.get(k)

    def contacts(self, e):
        return self.o.contacts(e)

    def warm_cache(self):
        return self.o.warm_cache()

    def substep(self, last=True):
        self.o.substep(last=last)

    def publish(self):
        self.o.publish()

    def physics_step(self):
        for sub in range(int(self.o.cfg.substeps)):
            self.substep(last=sub == int(self.o.cfg.substeps) - 1)
        self.publish()


class _NoVelocityTerms(_StandIn):
    """(a) The numpy integrator in float32 with b(q, 0) in place of b(q, qd), clamped by the rule; the box is the fp32 oracle's."""

    def __init__(self, sc, ms, velocity_terms=False):
        super().__init__(sc, ms)
        self.ms, self.h, self.velocity_terms = ms, float(sc.dt) / int(sc.substeps), velocity_terms

    def substep(self, last=True):
        st = {k: self.o.get(k) for k in ("q", "qd", "targets")}
        self.o.substep(last=last)
        qw, qdw = _implicit_pd_step(self.o, self.ms, self.h, st, np.float32, self.velocity_terms)
        lo, hi = (x[:, None] for x in ws.limits(self.ms))
        self.o.set("q", np.clip(qw, lo, hi))
        self.o.set("qd", np.where(qw < lo, np.maximum(qdw, 0), np.where(qw > hi, np.minimum(qdw, 0), qdw)))


class _ClampKeepsSpeed(_StandIn):
    """(c) The widened fp32 oracle with q clipped in numpy but qd kept: a clamp that does not stop the joint."""

    def __init__(self, sc, ms):
        super().__init__(*_variant("BlindGrasping", int(sc.num_envs), widen=WIDEN))
        self.lim = [x[:, None] for x in ws.limits(ms)]

    def substep(self, last=True):
        self.o.substep(last=last)
        self.o.set("q", f32(np.clip(self.o.get("q"), *self.lim)))


class _WrongQuadrant(_StandIn):
    """(d) The fp32 oracle fed pi - q for the first thumb joints beyond pi / 2 (speed and target mirrored with it, and all three
    mirrored back on the way out): the joint's sine is kept and its cosine negated, as a wrong quadrant selection would."""

    def set(self, k, v):
        v = np.array(v, dtype=np.float64)
        if k == "q":
            self.flip = v[THUMB] > 0.5 * np.pi
        if k in ("q", "targets"):
            v[THUMB] = np.where(self.flip, f32(np.pi - v[THUMB]), v[THUMB])
        if k == "qd":
            v[THUMB] = np.where(self.flip, -v[THUMB], v[THUMB])
        self.o.set(k, v)

    def get(self, k):
        v = self.o.get(k)
        if k in ("q", "targets"):
            v[THUMB] = np.where(self.flip, np.pi - v[THUMB], v[THUMB])
        if k == "qd":
            v[THUMB] = np.where(self.flip, -v[THUMB], v[THUMB])
        return v


def _margin(report):
    """By how many bounds the worst field of a report misses (<= 1: inside)."""
    return max(max(r[1] / (pr.C_RULE * r[0] + 1e-7), r[3] / (pr.C_RULE * r[2] + 1e-6)) for r in report.values())


def _refused(check):
    try:
        check()
    except AssertionError:
        return True
    return False


def test_fp32_oracle_in_the_kernels_place_passes():
    """The fp32 oracle itself, through the functions the GPU tests call: teacher-forced sub-steps of both kinds, both tasks and the
    `all` model, the published quantities, the free-running physics step."""
    from oracle.oracle import Oracle
    for task, name in (("BlindGrasping", None), ("BaseTask", None), ("BlindGrasping", "all"), ("BlindGrasping", "generic")):
        sc, _, ms = _setup(task, N, name)
        for kind in KINDS:
            r = _check_teacher(lambda: Oracle(sc, ms), kind, N, task, name)
            assert _margin(r) <= 1.0 / pr.C_RULE + 1e-12                       # it IS the fp32 reference
    sc, _, ms = _setup("BlindGrasping", N)
    for kind in KINDS:
        _check_published(lambda: Oracle(sc, ms), kind, N)
    _check_physics_step(lambda: _StandIn(sc, ms), N)


def test_each_new_dimension_bites():
    """Item 4.  Each stand-in is refused by the comparison functions of the GPU tests, and misses by the margin recorded here
    (difference / bound of its worst field over the three teacher-forced sub-steps; measured at N = 256, seed 11):
      (a) no velocity terms in the bias force    `free` 517 bounds (qd; the same integrator WITH them: 0.32, it passes)
      (b) one finger joint's hi lowered by 1e-3  `stops` 2.2e3 bounds (q), and the joint is not on its stop
      (c) a clamp that does not stop the joint   `stops` 5.1e5 bounds (qd), and the clamped joints still move
      (d) pi - q on the first thumb joint        `free` 2.6e4 bounds (qd); published quantities 9.9e4 bounds (site_pose)
    A kernel with one of these defects would therefore fail; the thresholds below are a tenth of the measured margins."""
    sc, _, ms = _setup("BlindGrasping", N)
    full = _run_teacher(lambda: _NoVelocityTerms(sc, ms, velocity_terms=True), "free", N)[1]
    pr.assert_c_rule(full, "numpy integrator in float32, b(q, qd)")           # the integrator itself is inside the bound ...
    rec = _teacher_ref("stops", N)[0]
    assert rec["at_hi"][LOWERED].sum() >= 5                                     # (b) lowers a limit that joints of the sample sit on
    low = _variant("BlindGrasping", N, lower=LOWERED)
    cases = {
        "a": ("free", lambda: _NoVelocityTerms(sc, ms), 51.0),                  # ... and without the velocity terms it is not
        "b": ("stops", lambda: _StandIn(*low), 220.0),
        "c": ("stops", lambda: _ClampKeepsSpeed(sc, ms), 5e4),
        "d": ("free", lambda: _WrongQuadrant(sc, ms), 2.6e3),
    }
    margins = {"a, with the velocity terms": _margin(full)}
    for key, (kind, make, least) in cases.items():
        assert _refused(lambda: _check_teacher(make, kind, N)), f"stand-in ({key}) passes the teacher-forced comparison"
        margins[key] = _margin(_run_teacher(make, kind, N, exact=False)[1])
        assert margins[key] >= least, (key, margins[key])
    assert _refused(lambda: _check_published(cases["d"][1], "free", N)), "stand-in (d) passes the published quantities"
    margins["d, published"] = _margin(_published_report(cases["d"][1], "free", N))
    assert margins["d, published"] >= 1e4
    assert _refused(lambda: _check_physics_step(cases["c"][1], N)), "stand-in (c) passes the free-running physics step"
    for key in ("b", "c"):                                                      # the exact assertion alone refuses them as well
        b, _ = _run_teacher(cases[key][1], "stops", N, exact=False)
        last = _teacher_ref("stops", N)[-1]
        assert _refused(lambda: _assert_on_the_stops(_snap(b, "BlindGrasping"), last["at_lo"], last["at_hi"], *ws.limits(ms))), key
    print("\nstand-ins, difference / bound of the worst field: " + ", ".join(f"({k}) {v:.3g}" for k, v in margins.items()))


# ------------------------------------------------------------------------------------------------- GPU
def _hip(n, fused=True, task="BlindGrasping", name=None):
    sc, _, ms = _setup(task, n, name)
    return pr.hip(sc, ms, fused)


FORMS = pytest.mark.parametrize("fused", [True, False], ids=["k_substep", "k_dynamics+k_solve"])
CASES = pytest.mark.parametrize("kind,n,task", [("free", N, "BlindGrasping"), ("stops", N, "BlindGrasping"), ("free", PADDED, "BlindGrasping"),
                                                ("stops", PADDED, "BlindGrasping"), ("stops", N, "BaseTask")],
                                ids=["free", "stops", "free-padded", "stops-padded", "stops-basetask"])


# Measured on one MI355X, ratios |HIP - fp64| / |fp32 oracle - fp64| at the 99.9th percentile / at the maximum over the three
# sub-steps, next to the fp32 oracle's own figures (the whole table, the padded runs and the `all` model: DESIGN.md, section 5);
# C_RULE allows 3.  Contact counts exact, every clamped joint on its float32 limit with qd = 0, no env left out.
#              free: fp32 oracle   k_substep    k_dynamics+k_solve   stops: fp32 oracle  k_substep    k_dynamics+k_solve
#   q          1.2e-7 / 1.2e-7     1.00 / 1.00  1.00 / 1.00          1.2e-7 / 1.2e-7     1.00 / 1.00  1.00 / 1.00
#   qd         3.2e-6 / 5.6e-6     0.61 / 0.79  0.61 / 0.79          2.6e-6 / 3.5e-6     0.72 / 1.25  0.72 / 1.25
#   box_pos    6.6e-10             1.00 / 1.00  1.00 / 1.00          6.6e-10             1.00 / 1.00  1.00 / 1.00
#   box_quat   1.3e-9              1.00 / 1.00  1.02 / 1.02          1.3e-9              1.00 / 1.00  1.02 / 1.02
#   box_lin    2.6e-8              1.01 / 1.01  1.03 / 1.03          2.6e-8              1.01 / 1.01  1.03 / 1.03
#   box_ang    1.1e-6              1.00 / 1.00  1.02 / 1.02          1.1e-6              1.00 / 1.00  1.02 / 1.02
#   cforce     1.1e-6              1.01 / 1.01  1.02 / 1.02          1.1e-6              1.01 / 1.01  1.02 / 1.02
#   wlam 80-83 1.7e-9              0.81 / 0.81  0.90 / 0.90          1.7e-9              0.81 / 0.81  0.90 / 0.90
# BaseTask, stops, both forms: q 1.00 / 1.00, qd 0.79 / 0.83 against 2.6e-6 / 4.5e-6.
@pytest.mark.gpu
@FORMS
@CASES
def test_teacher_forced_substeps_at_wide_poses(kind, n, task, fused):
    _check_teacher(lambda: _hip(n, fused, task), kind, n, task)


@pytest.mark.gpu
@FORMS
@CASES
def test_published_quantities_at_wide_poses(kind, n, task, fused):
    _check_published(lambda: _hip(n, fused, task), kind, n, task)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N, PADDED], ids=["256", "200-padded"])
def test_one_fused_physics_step_from_the_stops(n):
    _check_physics_step(lambda: _hip(n), n)


HIP_STATE = pr.SYNC + ("cforce", "site_pose", "hand_vel", "ncontact", "wlam", "wgen")


@pytest.mark.gpu
def test_fused_physics_launch_is_four_substep_launches_and_reproducible():
    """Bit for bit on the `stops` sample: k_physics4 against four single sub-step launches, and two instances against each other."""
    import torch
    from dexrobot_isaac_amd import _abi
    st = _state("stops", N)
    a, b, c = _hip(N), _hip(N), _hip(N)
    for x in (a, b, c):
        pr.load(x, st)
    a.core.run_stage(_abi.STAGE["PHYSICS"]), c.core.run_stage(_abi.STAGE["PHYSICS"])
    for _ in range(int(_setup("BlindGrasping", N)[0].substeps)):
        b.core.run_stage(_abi.STAGE["SUBSTEP"])
    torch.cuda.synchronize()
    lo, hi = ws.limits(_setup("BlindGrasping", N)[2])
    q = a.get("q")
    assert ((q == lo[:, None]) | (q == hi[:, None]))[6:].sum() >= 500            # the step really ended with joints on their stops
    for f in HIP_STATE:
        assert torch.equal(a.core.field(f), c.core.field(f)), f"two instances differ in {f}"
    for f in HIP_STATE:
        if f not in ("site_pose", "hand_vel"):                                   # (a single sub-step launch publishes nothing)
            assert torch.equal(a.core.field(f), b.core.field(f)), f"the fused launch differs from four sub-step launches in {f}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_specialised_kernels_equal_the_general_ones_at_wide_poses(kind):
    """The model structure folded out of the chains (tests/test_model_structure.py) removes exact zeros and ones: `==` over the three
    teacher-forced sub-steps, where the velocity products and the base rotations are no longer small."""
    import torch
    spec = _hip(N)
    with pr.general_path():
        gen = _hip(N)
    for sub, rec in enumerate(_teacher_ref(kind, N)):
        for b in (spec, gen):
            pr.load(b, rec["start"])
            b.substep(last=True)
        torch.cuda.synchronize()
        for f in pr.SYNC + ("cforce", "ncontact", "wlam"):
            assert torch.equal(spec.core.field(f), gen.core.field(f)), f"sub-step {sub}: {f} differs"
    for b in (spec, gen):
        b.publish()
    torch.cuda.synchronize()
    for f in PUBLISHED:
        assert torch.equal(spec.core.field(f), gen.core.field(f)), f"published {f} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_general_kernels_on_the_model_without_structure_at_wide_poses(kind):
    """The `all` model of tests/test_model_structure.py lacks every folded property and runs the general kernels, which were held
    only to the free-running median / 99th-percentile bars: the sample drawn for it, the rule of the teacher-forced test against the
    oracles of that model."""
    _check_teacher(lambda: _hip(N, name="all"), kind, N, name="all")
    _check_published(lambda: _hip(N, name="all"), kind, N, name="all")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_general_kernels_on_the_generic_model_at_wide_poses(kind):
    """The same on the `generic` model (tests/generic_model.py), which lacks every zero, one and repeated number of the default model by
    tenths of a radian and a centimetre, not by the 1e-2 rad and millimetres that flip the classification: every term of the
    general chains carries weight.  test_sample_covers_the_cases_generic_model holds the conditions of the sample."""
    _check_teacher(lambda: _hip(N, name="generic"), kind, N, name="generic")
    _check_published(lambda: _hip(N, name="generic"), kind, N, name="generic")
