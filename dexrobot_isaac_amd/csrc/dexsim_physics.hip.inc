// dexsim_physics.hip.inc -- the physics kernels (included by dexsim.hip).
//
// Replaces gym.simulate + gym.fetch_results (reference components/physics/physics_manager.py:92-99) for the
// 26-DOF fixed-base DexHand + free box + ground plane.  One env per lane, 64 envs per wavefront, lockstep.
//
//   k_physics4 / k_physics1 (substep_body): the production path -- four sub-steps or one sub-step in one launch (a physics
//                step is substeps / 4 launches of k_physics4, then substeps % 4 of k_physics1), seven wavefronts per 64 envs:
//                articulated dynamics in block / Schur form (CRBA in momentum form finger by finger, RNEA bias, implicit-PD
//                factorisation
//                  Mhat = [B C; C^T F] = L^T diag(S, F_0..F_4) L ,  L = [I 0; G I],  G_f = Fhat_f^-1 C_f^T),
//                free velocity in the decoupled coordinates u = L qd, capsule / box / plane narrowphase, contact rows in
//                u-space (t = j_B - G_f^T j_f, S^-1 t, Fhat_f^-1 j_f, 1/D), the warm-started block solver (every hand
//                contact a work item), back-substitution qd = L^-1 u, integration, publication.
//   k_dynamics + k_solve : the un-fused ancestors (dynamics + rows | contact solve + integration) as stand-alone kernels, kept
//                for staged parity tests and for timing the contact solve in isolation (the "contact-solve kernel" of
//                BASELINE.json); k_solve's general path is a plain one-wave restatement of the block solver.
//   k_publish  : FK of the 11 sites, hand-base twist, AoS dof_state / root_state publication
//                (gym.refresh_*_tensor, physics_manager.py:106-109).
//
// The arithmetic model is specified by oracle/dexsim_oracle.c (dense form); this file is its block-structured
// MI355X implementation.

// LDS row store of the contact solver: word w of the lane's row data lives at [w / 4][lane][w % 4], so that a lane reads
// four consecutive row words with one 16-byte ds_read_b128 (conflict-free: 64 lanes x 16 B).  A contact's 3 x 28 words are
// 21 LDS instructions instead of 84 -- a wave has at most 15 LDS instructions in flight, so the count sets the latency.
#define ROWADDR(w, lane) ((((w) >> 2) * 64 + (lane)) * 4 + ((w) & 3))

// Role of hardware wave w of a 7-wave workgroup: 0-4 = finger, 5 = palm + base joints, 6 = box.  Waves are placed round-robin
// on the CU's four SIMDs (w % 4), so three SIMDs carry two waves.  The two light roles -- palm and box -- share SIMD 2 (waves 2
// and 6), fingers pair up on SIMDs 0 and 1 and finger 2 has SIMD 3 to itself: the box wave's speculative contact solve then
// competes for issue slots only with the palm wave, which is done after a third of phase 1.
DI int wave_role(int w) { return w == 2 ? 5 : ((w >= 3 && w <= 5) ? w - 1 : w); }
#ifndef SPEC_SPLIT_NUM
#define SPEC_SPLIT_NUM 12   /* of the 16 box/ground sweeps, the share (x/16) run speculatively in phase 1 (substep_body); 9 until the Schur phase was
                               split over four waves, 13 until round 3 shortened the finger waves' phase 1 (quad hand-off, diagonal inertias) and
                               the box wave became the last to reach the phase-1 barrier: 13 -> 12: 63.5 -> 64.1 M env-steps/s, 11 = 13, 10 slower */
#endif

// sw >= 0: parallel narrowphase of the fused sub-step -- wave sw collects the contacts of its own capsules in its staging
// block of the arena (15 contacts x 9 words: geometry + code); they are appended to the list in the fixed priority order
// once every wave's count is known (substep_body, phase 2).  nc then counts the wave's local contacts.
// contact code: bits [1:0] type (0 hand/ground, 1 hand/box, 2 box/ground), [6:2] capsule, [9:7] sample (hand contacts: 0 / 1 =
// which point of the capsule; box/ground: the corner index), [14:12] the finger's split count (build_contact_rows)
#define CODE_TYPE(c) ((c) & 3)
#define CODE_CAP(c) (((c) >> 2) & 31)
#define CODE_SAMPLE(c) (((c) >> 7) & 7)
// [18:16] finger of the capsule + 1 (0: palm / none), [20:19] its joint's level in the finger, [25:21] force slot of its body: model
// look-ups made where the capsule index is wave-uniform (narrowphase), so that the row builder starts without dependent loads
#define CODE_FINGER(c) ((((c) >> 16) & 7) - 1)
#define CODE_LEVEL(c) (((c) >> 19) & 3)
#define CODE_FSLOT(c) (((c) >> 21) & 31)
DI int code_info(const DexHandModel& M, int cap) {
  const int jp = M.cap_parent[cap];
  return ((jp >= 6 ? ((jp - 6) >> 2) + 1 : 0) << 16) | ((jp >= 6 ? (jp - 6) & 3 : 0) << 19) | (M.cap_fslot[cap] << 21);
}
// warm-start cache slot of a contact: hand contacts by (capsule, type, sample); box/ground contacts by LIST SLOT k (80 + k) with
// the corner in the tag (see the box wave's phase 1)
#define CODE_HKEY(c) (CODE_TYPE(c) == 3 ? 88 + ((CODE_FINGER(c) * 4 + CODE_LEVEL(c)) * 2 + (CODE_SAMPLE(c) & 1)) \
                                         : (CODE_CAP(c) * 2 + CODE_TYPE(c)) * 2 + (CODE_SAMPLE(c) & 1))
// type 3 = joint-limit row (cfg.joint_limit_rows; specification: oracle/dexsim_oracle.c push_limit_rows): a one-row speculative
// constraint J = +-e_j on finger joint j = (CODE_FINGER, CODE_LEVEL), CODE_SAMPLE = side (0 lower: +e_j, 1 upper: -e_j), gap = distance
// to the limit, no friction, no geometry (p = n = 0).  It is a hand block of its finger like a contact; it is not a contact in the
// statistics and exerts no body force.
// Split counts of a lane's env, packed (phase 2: wave 0 -> FS_SPLIT; k_dynamics: wave 5 -> DL_SPLIT): bits [3:0] nB = solver blocks
// with hand contacts (<= 12), [7:4] nX = blocks touching the box, [11:8] .. [27:24] nF of finger 0 .. 4 = blocks holding contacts of
// that finger, [28] log2 of the run length (0: every hand contact its own block, 1: pairs)
#define SPLIT_NB(s) ((s) & 15)
#define SPLIT_NX(s) (((s) >> 4) & 15)
#define SPLIT_NF(s, f) (((s) >> (8 + 4 * (f))) & 15)
#define SPLIT_RS(s) (((s) >> 28) & 1)
// word the narrowphase waves exchange in phase 2 (token words FS_FLAG + w): bit 0 = the wave's broadphase verdict, UNCHANGED (a
// wave that is late out of the phase-1 barrier still builds its clear_mask from bit 0 of these words: the rewrite must not be
// able to flip it), bits [7:1] local contact count, [22:8] which of them are hand/box contacts; the tag bit keeps the word from
// ever looking like a broadphase token of a later sub-step
#define NP_TAG 0x40000000
#define NP_COUNT(w) (((w) >> 1) & 0x7f)
#define NP_TMASK(w) (((w) >> 8) & 0x7fff)
// The packed split counts from: nbg box/ground contacts, cnt[w] hand contacts of finger w = 0..4 / the palm (w = 5) in list
// order (already cut to KMAX), hmask = which hand contacts (bit = hand index) touch the box.
DI int split_pack(int nbg, const int (&cnt)[6], int hmask) {
  int nh = 0;
#pragma unroll
  for (int w = 0; w < 6; w++) nh += cnt[w];
  const int rs = nh > 12 ? 1 : 0;
  int split = max(1, (nh + rs) >> rs) | (rs << 28);
  int a = 0;
#pragma unroll
  for (int w = 0; w < 6; w++) {
    if (w < 5) split |= (cnt[w] > 0 ? (((a + cnt[w] - 1) >> rs) - (a >> rs) + 1) : 1) << (8 + 4 * w);
    a += cnt[w];
  }
  const int bmask = rs ? ((hmask | (hmask >> 1)) & 0x555555) : hmask;   // one bit per block that touches the box
  const int nX = (nbg > 0 ? 1 : 0) + __popc(bmask);
  return split | (max(nX, 1) << 4);
}
DI void push_contact(const Arena& A, int N, int e, int& nc, int type, int cap, int sample, V3 p, V3 n, float gap, float mu, int sw = -1,
                     int* tmask = nullptr, int cinfo = 0) {
  if (sw >= 0) {
    if (nc >= NP_STAGE) return;
    if (tmask && type == 1) *tmask |= 1 << nc;
    // staging block: 2 quads per contact (FQ layout: p.xyz n.x | n.yz gap mu), the codes as plain rows behind the 180 quads
    const int sc = sw * NP_STAGE + nc;
    *FQ(cstage, 2 * sc) = f4{p.x, p.y, p.z, n.x};
    *FQ(cstage, 2 * sc + 1) = f4{n.y, n.z, gap, mu};
    FLD(cstage, CSTAGE_CODE0 + sc) = __int_as_float(type | (cap << 2) | (sample << 7) | cinfo);
    nc++;
    return;
  }
  if (nc >= DEXSIM_KMAX) return;
  if (tmask && type == 1) *tmask |= 1 << nc;
  *FQ(cgeom, 2 * nc) = f4{p.x, p.y, p.z, n.x};       // manifold entry: 2 quads (FQ layout), like the staging block
  *FQ(cgeom, 2 * nc + 1) = f4{n.y, n.z, gap, mu};
  FLD(ccode, nc) = type | (cap << 2) | (sample << 7) | cinfo;
  nc++;
}

// one capsule against the box (closest point of the axis + its far end, as sample spheres) and the ground (both ends)
// (k_dynamics only.  Kept next to collide_capsules3: with k_dynamics on that one, 10-60 instructions of every k_physics* kernel
// sit elsewhere -- same registers, same instruction multiset -- and the headline measured 0.5-0.9 % slower in 6 of 6 alternating runs.)
DI void collide_capsule(const Arena& A, int N, int e, int& nc, const DexSimConfig& C, int cap, V3 e0, V3 e1, float r,
                        bool has_box, V3 bpos, const M3& Rb, float hb, float mu_hb, float mu_hg, int sw = -1, int* tmask = nullptr, int cinfo = 0) {
  const float co = C.contact_offset, rest = C.rest_offset;
  if (has_box) {
    V3 a = mulT(Rb, e0 - bpos), b = mulT(Rb, e1 - bpos), d = b - a;
    V3 mid = {0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z)};
    float reach = 0.5f * norm_n(d) + r + 1.7320508f * hb + co;   // d: a capsule axis of the model (exactly zero for a sphere)
    // broadphase (bounding spheres); wave-level early-out keeps the lockstep lanes from paying for the
    // bisection when no env in the wavefront is near its box
    bool near = dot(mid, mid) < reach * reach;
    if (__any(near)) {
      if (near) {
        float lo = 0.f, hi = 1.f;
#pragma unroll 4
        for (int it = 0; it < DEXSIM_BISECT_ITERS; it++) {
          float mdl = 0.5f * (lo + hi);
          if (seg_box_dfdt(a, d, mdl, hb) > 0.f) hi = mdl; else lo = mdl;
        }
        float ts = 0.5f * (lo + hi);
        // closest feature first: the point of the axis nearest to the box (snapped to an end within 2 % of it), then at
        // most one more sample -- the far end of the axis, which only passes the gap test when the capsule lies along
        // the surface (a line contact needs two points to be stable).  At most 2 contacts per capsule/box pair.
        const float tp = ts <= 0.02f ? 0.f : (ts >= 0.98f ? 1.f : ts);
        for (int s = 0; s < 2; s++) {
          float tc = s == 0 ? tp : (tp < 0.5f ? 1.f : 0.f);
          V3 Pc = {a.x + tc * d.x, a.y + tc * d.y, a.z + tc * d.z}, nl, pl;
          float gr;
          sphere_box(Pc, r, hb, nl, pl, gr);
          if (gr < co) push_contact(A, N, e, nc, 1, cap, s, mul(Rb, pl) + bpos, mul(Rb, nl), gr - rest, mu_hb, sw, tmask, cinfo);
        }
      }
    }
  }
  float z0 = e0.z - r, z1 = e1.z - r;
  if (z0 < co) push_contact(A, N, e, nc, 0, cap, 0, v3(e0.x, e0.y, z0), v3(0, 0, 1), z0 - rest, mu_hg, sw, tmask, cinfo);
  if (z1 < co) push_contact(A, N, e, nc, 0, cap, 1, v3(e1.x, e1.y, z1), v3(0, 0, 1), z1 - rest, mu_hg, sw, tmask, cinfo);
}

// Three capsules of one wave (a finger's, or the palm's) in the order given -- collide_capsule three times, but with the three
// bisections interleaved in one loop: each is a chain of 16 dependent steps of ~20 instructions, and a lone wave issues a
// dependent instruction only every ~8 cycles; three independent chains fill each other's gaps.  Same arithmetic per capsule,
// same contact order.
DI void collide_capsules3(const Arena& A, int N, int e, int& nc, const DexSimConfig& C, const int (&cap)[3], const V3 (&E0)[3],
                          const V3 (&E1)[3], const float (&r)[3], bool has_box, V3 bpos, const M3& Rb, float hb, float mu_hb, float mu_hg,
                          int sw, int* tmask, const int (&cinfo)[3]) {
  const float co = C.contact_offset, rest = C.rest_offset;
  V3 a[3], d[3];
  bool near[3] = {false, false, false};
  float ts[3] = {0.f, 0.f, 0.f};
  if (has_box) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      a[c] = mulT(Rb, E0[c] - bpos);
      const V3 b = mulT(Rb, E1[c] - bpos);
      d[c] = b - a[c];
      const V3 mid = {0.5f * (a[c].x + b.x), 0.5f * (a[c].y + b.y), 0.5f * (a[c].z + b.z)};
      const float reach = 0.5f * norm_n(d[c]) + r[c] + 1.7320508f * hb + co;   // d: a capsule axis of the model (exactly zero for a sphere)
      near[c] = dot(mid, mid) < reach * reach;      // broadphase (bounding spheres)
    }
    // (Round 3 guarded each capsule's chain with its own wave-uniform "some lane is near" branch: no measurable change in any regime
    // -- 91.3 vs 91.3 us near-but-not-touching, 13.56 vs 13.57 M env-steps/s training-like -- the chains are not what this phase waits for.)
    if (__any(near[0] || near[1] || near[2])) {
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f};
#pragma unroll 2
      for (int it = 0; it < DEXSIM_BISECT_ITERS; it++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const float mdl = 0.5f * (lo[c] + hi[c]);
          if (seg_box_dfdt(a[c], d[c], mdl, hb) > 0.f) hi[c] = mdl; else lo[c] = mdl;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++) ts[c] = 0.5f * (lo[c] + hi[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const V3 ac = a[c], dc = d[c], e0 = E0[c], e1 = E1[c];
    const float rc = r[c], tsc = ts[c];
    const bool nr = near[c];
    const int capc = cap[c], ci = cinfo[c];
    if (has_box && nr) {
      // closest feature first, then at most one more sample -- the far end of the axis (see collide_capsule)
      const float tp = tsc <= 0.02f ? 0.f : (tsc >= 0.98f ? 1.f : tsc);
      for (int s = 0; s < 2; s++) {
        const float tc = s == 0 ? tp : (tp < 0.5f ? 1.f : 0.f);
        V3 Pc = {ac.x + tc * dc.x, ac.y + tc * dc.y, ac.z + tc * dc.z}, nl, pl;
        float gr;
        sphere_box(Pc, rc, hb, nl, pl, gr);
        if (gr < co) push_contact(A, N, e, nc, 1, capc, s, mul(Rb, pl) + bpos, mul(Rb, nl), gr - rest, mu_hb, sw, tmask, ci);
      }
    }
    const float z0 = e0.z - rc, z1 = e1.z - rc;
    if (z0 < co) push_contact(A, N, e, nc, 0, capc, 0, v3(e0.x, e0.y, z0), v3(0, 0, 1), z0 - rest, mu_hg, sw, tmask, ci);
    if (z1 < co) push_contact(A, N, e, nc, 0, capc, 1, v3(e1.x, e1.y, z1), v3(0, 0, 1), z1 - rest, mu_hg, sw, tmask, ci);
  }
}

// ------------------------------------------------------------------------------------------------- dynamics
// k_dynamics, version 2: one workgroup = 6 wavefronts x 64 lanes for 64 envs (lane = env in every wave).
//   wave f = 0..4 : finger f  -- FK, CRBA blocks F_f / C_f, RNEA bias, Fhat_f^-1, G_f, u_free of the finger
//   wave 5        : palm + box -- palm composite/wrench, box free velocity, box/ground contacts, then the
//                   narrowphase of all capsules (in the oracle's fixed priority order)
// hand-off through LDS [word][lane]; wave 0 then reduces the five Schur contributions, inverts S (6x6) and writes
// u_B; contact rows are finally built by all six waves, contact k on wave k % 6.
// Version 1 ran the five fingers sequentially in one wave (64 us at N=4096, a single wave per CU); the fingers
// are independent sub-trees given the base chain, so they map onto separate wavefronts without changing the
// arithmetic.  Every wave recomputes the 6-joint base chain (cheap) instead of synchronising on it.
// (LDS words: the LDS map below.)

struct BaseChain {
  V3 ab[6], ob[6];
  float qb[6], qdb[6];
  Q4 q5;
  V3 o5, w5, al5, ao5;
};

// Joints 0-2 are prismatic and joint 3 is the first revolute one, so everything up to joint frame 3 at q3 = 0 is a
// constant of the model: world axes A_j, origins Oc_j + sum q_i A_i, no angular velocity / acceleration yet (the
// generic recursion spent ~700 of its ~1100 instructions per wave and sub-step on these constants and on cross
// products with w = alpha = 0).  dexsim_create folds them in double precision (DevParams::base_*); joints 4, 5 stay generic.
// s_q / s_qd (fused kernel, bodies 2-4): q, qd of the base joints from the LDS words the palm wave left there at the end of the
// previous body, instead of from the arena (an L2 round trip behind that body's stores)
//
// Model structure (template parameter MS of the step kernels).  The chains multiply by model constants that are exactly zero or
// one, which the compiler cannot know: they arrive through s_load, and without nsz / nnan it may not fold x * 0 anyway.
// dexsim_create classifies the model's floats by exact comparison and picks the kernel, so the chains stay straight-line code (a
// wave-uniform dispatch between two copies of the finger chain inside one kernel cost 14 VGPRs and 112 B of scratch).  MS holds when
//   base     joints 4 and 5 have identity qoff, zero poff and axes +e_y / +e_z (joint frames 3-5 share one origin), and the world
//            axes base_A[0..2] of the prismatic joints are exactly e_x, e_y, e_z;
//   fingers  joints 1-3 of every finger have axis +-e_y.
// Every dropped term is an exact zero and every dropped factor an exact one, so a result equals the general form's for finite
// inputs (the sign of an exact zero may differ).  Where two products survive, the form spells out the rounding sequence the
// general expression compiles to (-ffp-contract=fast): one product rounded on its own (mulr), the other fused onto it (fmaf).
// Which of two products the compiler rounds depends on the expression AND its surroundings, so every form here was read off the
// general kernel's code at that site and is pinned by tests/test_model_structure.py (`==` against the general kernels).  Forms
// that could not be kept equal (the finger joints' identity qoff, one-component axis quaternion, poff and com along x) are
// listed in profiles/model_structure/README.md: a specialised joint changes how the compiler contracts the q2mat next to it.
// qmul(a, {0, s, 0, c}) and qmul(a, {0, 0, s, c}): a joint rotation about e_y / e_z
DI Q4 qmul_axis_y(Q4 a, float s, float c) {
  return {fmaf(-a.z, s, mulr(a.x, c)), fmaf(a.y, c, mulr(a.w, s)), fmaf(a.z, c, mulr(a.x, s)), fmaf(-a.y, s, mulr(a.w, c))};
}
DI Q4 qmul_axis_z(Q4 a, float s, float c) {
  return {fmaf(a.y, s, mulr(a.x, c)), fmaf(a.y, c, -mulr(a.x, s)), fmaf(a.z, c, mulr(a.w, s)), fmaf(-a.z, s, mulr(a.w, c))};
}
// columns y and z of q2mat(q), in the rounding order of the general base chain's q2mat at joints 4 and 5
DI V3 q2mat_col_y(Q4 q) {
  return {2.f * fmaf(q.x, q.y, -mulr(q.z, q.w)), fmaf(fmaf(q.z, q.z, mulr(q.x, q.x)), -2.f, 1.f), 2.f * fmaf(q.y, q.z, mulr(q.x, q.w))};
}
DI V3 q2mat_col_z(Q4 q) {
  return {2.f * fmaf(q.x, q.z, mulr(q.y, q.w)), 2.f * fmaf(q.y, q.z, -mulr(q.x, q.w)), fmaf(fmaf(q.y, q.y, mulr(q.x, q.x)), -2.f, 1.f)};
}

// MS: frame j = 4, 5 sits on frame j - 1 (identity qoff, no lever arm), its axis e_y / e_z is a column of that frame's rotation
template <bool MS>
DI void base_chain(const Arena& A, const DevParams* __restrict__ P, V3 grav, int N, int e, BaseChain& B, bool write_jframe,
                   const float* s_q = nullptr, const float* s_qd = nullptr, int lane = 0) {
  // all loads before the (conditional) jframe stores below: a load cannot be hoisted above a possibly aliasing store
#pragma unroll
  for (int j = 0; j < 6; j++) {
    if (s_q) { B.qb[j] = s_q[j * 64 + lane]; B.qdb[j] = s_qd[j * 64 + lane]; }
    else { B.qb[j] = FLD(q, j); B.qdb[j] = FLD(qd, j); }
  }
  V3 t = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const V3 Aj = v3p(P->base_A[j]);
    if (j < 3) t += B.qb[j] * Aj;
    B.ab[j] = Aj;
    B.ob[j] = v3p(P->base_Oc[j]) + t;
  }
  Q4 qc;
  {
    const V3 ax = v3p(P->jc[3].axis);
    float s, c;
    sincos_joint(0.5f * B.qb[3], &s, &c);
    qc = qmul(q4p(P->base_Q3z), Q4{ax.x * s, ax.y * s, ax.z * s, c});
  }
  V3 oc = B.ob[3];
  V3 w = B.qdb[3] * B.ab[3], al = {0, 0, 0}, ao = {-grav.x, -grav.y, -grav.z};
#pragma unroll
  for (int j = 4; j < 6; j++) {
    if (MS) {
      const V3 aw = j == 4 ? q2mat_col_y(qc) : q2mat_col_z(qc);
      float s, c;
      sincos_joint(0.5f * B.qb[j], &s, &c);
      const Q4 qn = j == 4 ? qmul_axis_y(qc, s, c) : qmul_axis_z(qc, s, c);
      const V3 cw = cross(w, aw);
      al += B.qdb[j] * cw; w += B.qdb[j] * aw;
      B.ab[j] = aw; B.ob[j] = oc; qc = qn;
      continue;
    }
    M3 Rp = q2mat(qc);
    V3 on = oc + mul(Rp, v3p(P->jc[j].poff));
    Q4 qz = qmul(qc, q4p(P->jc[j].qoff));
    V3 ax = v3p(P->jc[j].axis);
    V3 aw = mul(q2mat(qz), ax);
    float s, c;
    sincos_joint(0.5f * B.qb[j], &s, &c);
    Q4 qn = qmul(qz, Q4{ax.x * s, ax.y * s, ax.z * s, c});
    V3 r = on - oc;
    V3 aoj = ao + cross(al, r) + cross(w, cross(w, r));
    V3 cw = cross(w, aw);
    al += B.qdb[j] * cw; w += B.qdb[j] * aw;
    ao = aoj; B.ab[j] = aw; B.ob[j] = on; qc = qn; oc = on;
  }
  B.q5 = qc; B.o5 = oc; B.w5 = w; B.al5 = al; B.ao5 = ao;
  if (write_jframe) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      FLD(jframe, 6 * j + 0) = B.ab[j].x; FLD(jframe, 6 * j + 1) = B.ab[j].y; FLD(jframe, 6 * j + 2) = B.ab[j].z;
      FLD(jframe, 6 * j + 3) = B.ob[j].x; FLD(jframe, 6 * j + 4) = B.ob[j].y; FLD(jframe, 6 * j + 5) = B.ob[j].z;
    }
  }
}

// Hand-level broadphase: true when, for every env of the wavefront, no point of any hand capsule can be within the
// contact offset of the box or the ground (bounding sphere of radius hand_reach about the palm joint origin).  Every
// wave of the workgroup evaluates it on identical data, so the result is uniform over the workgroup.  When it holds
// the narrowphase, and the joint-frame / factor hand-off that only hand-contact rows read, are skipped.
DI bool hand_clear(const DevParams* __restrict__ P, const BaseChain& B, V3 bpos) {
  const DexSimConfig& C = P->cfg;
  const float reach = P->hand_reach, co = C.contact_offset;
  bool clear = B.o5.z - reach > co;
  if (C.has_box) {
    const V3 d = B.o5 - bpos;
    const float rr = reach + 0.8660254f * C.box_size * 1.001f + co;
    clear = clear && dot(d, d) > rr * rr;
  }
  return __all(clear);
}

// Second level of the broadphase, per capsule: the bounds collide_capsule itself applies before doing any work (ground:
// exactly its contact test; box: its bounding-sphere early-out, with a rounding margin).  A finger (or the palm) whose
// capsules all pass in every lane of the wavefront cannot produce a contact in this sub-step.
// Round 3: against the box the bound is the distance of the capsule's MIDPOINT to the box itself (clamped in the box frame) instead
// of to the box's bounding sphere: every point of the axis is within half the axis length of the midpoint, so a sample sphere can
// only be within the contact offset if dist(mid, box) < |d| / 2 + r + offset.  Still conservative (the narrowphase's own early-out
// is looser, its contact test is what it was), but the zone in which a workgroup takes the general path without any contact shrinks
// from the box's bounding sphere (43 mm beyond the faces at the face centres) to the capsule's own extent -- a hand approaching its
// box stays on the hand-clear path until a capsule is really about to touch.
DI bool capsule_clear(V3 e0, V3 e1, float r, const DexSimConfig& C, V3 bpos, const M3& Rb) {
  const float co = C.contact_offset;
  bool clear = !((e0.z - r) < co) && !((e1.z - r) < co);
  if (C.has_box) {
    const V3 d = e1 - e0;
    const V3 mid = mulT(Rb, V3{0.5f * (e0.x + e1.x) - bpos.x, 0.5f * (e0.y + e1.y) - bpos.y, 0.5f * (e0.z + e1.z) - bpos.z});
    const float hb = 0.5f * C.box_size;
    const V3 ex = {mid.x - clampf(mid.x, -hb, hb), mid.y - clampf(mid.y, -hb, hb), mid.z - clampf(mid.z, -hb, hb)};
    const float reach = (0.5f * norm_n(d) + r + co) * 1.0001f + 1e-6f;   // d: a capsule axis of the model (exactly zero for a sphere)
    clear = clear && !(dot(ex, ex) < reach * reach);
  }
  return clear;
}

#define SH(i) sh[(i) * 64 + lane]
DI void sh_put3(float* sh, int lane, int i, V3 v) { SH(i) = v.x; SH(i + 1) = v.y; SH(i + 2) = v.z; }
// A wave's composite body (a finger's, the palm's) as it is handed to the Schur phase: mass, centre of mass relative to the palm
// joint's origin o5, and the inertia about o5 (parallel axis) -- in that form the hand's composite is a plain sum over the six
// parts plus one shift back to the common centre of mass (~90 instructions on the Schur wave; summing centre-of-mass
// composites pair by pair, each with its own division and two parallel-axis shifts, was 4.2k of that wave's 9k cycles).
DI void comp_put(float* sh, int lane, int w, const Comp& c, V3 o5) {
  const V3 d = c.c - o5;
  const S6 J = c.I + pa(c.m, d);
  sh[(w) * 64 + lane] = c.m; sh_put3(sh, lane, w + 1, d);
  sh[(w + 4) * 64 + lane] = J.xx; sh[(w + 5) * 64 + lane] = J.yy; sh[(w + 6) * 64 + lane] = J.zz;
  sh[(w + 7) * 64 + lane] = J.xy; sh[(w + 8) * 64 + lane] = J.xz; sh[(w + 9) * 64 + lane] = J.yz;
}
DI V3 sh_get3(const float* sh, int lane, int i) { return {SH(i), SH(i + 1), SH(i + 2)}; }
// axes / origins of base joints 2 i2 and 2 i2 + 1 from the quad-layout block the palm wave leaves in LDS (s_bch = sh + FS_BCH * 64)
DI void bch_get2(const float* s_bch, int lane, int i2, V3& a0, V3& o0, V3& a1, V3& o1) {
  const f4 q0 = *(const f4*)(s_bch + ROWADDR(12 * i2, lane)), q1 = *(const f4*)(s_bch + ROWADDR(12 * i2 + 4, lane)),
           q2 = *(const f4*)(s_bch + ROWADDR(12 * i2 + 8, lane));
  a0 = {q0.x, q0.y, q0.z}; o0 = {q0.w, q1.x, q1.y}; a1 = {q1.z, q1.w, q2.x}; o1 = {q2.y, q2.z, q2.w};
}

// ---- LDS map of the sub-step kernels
// The waves of a workgroup hand data to each other through LDS laid out [word][lane]: word w of lane l is sh[w * 64 + l] (bank =
// lane: conflict-free for any per-lane index).  k_dynamics holds the persistent words, the per-finger hand-off at DL_PERSIST and
// its split word.  k_physics4 / k_physics1 own the CU's whole LDS (FS_WORDS words; one workgroup per CU, which the LDS token waits
// rely on, see substep_body), and most of their words serve two regions in turn.  LDS_MAP below lists every region of theirs with
// the phases in which it is live, from its first write to its last read on any path, and the compiler checks that no two regions
// live in a common phase share a word.  Sub-fields (DL_SCHUR_*, DL_PALM_WRENCH, FS_SPRE_BIAS, the hand-off's DL_*) lie inside
// their region.

// persistent words (k_dynamics and the fused kernels)
#define DL_SINV 0            /* 36: S^-1, 9 quads (ROWADDR layout) for the row builders; the hand-clear fused sub-step holds instead: */
#define DL_SCHUR_S 0         /*     21: S, lower triangle, from the split Schur phase (schur_helper, schur_row) */
#define DL_SCHUR_GSUM 27     /*      6: sum of G_f^T tau_f (schur_helper, job 1) */
#define DL_PALM 36           /* 16: the palm's composite (comp_put form, 10 words) and: */
#define DL_PALM_WRENCH 46    /*      6: its RNEA wrench about o5 */
#define DL_NC 52             /*  1: contact count (fused: | box/ground contacts << 8) */
#define DL_PERSIST 53
// per-finger hand-off of phases 1-2 at word b (k_dynamics: DL_PERSIST, fused: FS_ROW)
#define DL_SSUB(b, f) ((b) + (f) * 43)         /* 21: C_f G_f, lower triangle */
#define DL_GSUM(b, f) ((b) + (f) * 43 + 21)    /*  6: G_f^T tau_f */
#define DL_COMP(b, f) ((b) + (f) * 43 + 27)    /* 10: composite of the finger: m, c - o5, I about o5 (comp_put) */
#define DL_WRENCH(b, f) ((b) + (f) * 43 + 37)  /*  6: RNEA wrench about o5 */
#define DL_CAPS(b, f) ((b) + 215 + (f) * 18)   /* 18: 3 capsules x (e0, e1) */
#define DL_HANDOFF 305
#define DL_WORDS (DL_PERSIST + DL_HANDOFF)
#define DL_SPLIT DL_WORDS    /* k_dynamics: the env's split counts (wave 5, phase 2 -> the row builders) */

// the fused sub-step (k_physics4 / k_physics1), by word
#define FS_UB 53             /* u_B: free, then solved velocities of the base joints */
#define FS_BOXV 59           /* box twist (v, w): free, then solved */
#define FS_UF 65             /* u_f, word 4 f + l: free, then solved */
#define FS_LAM 85            /* impulses of the KMAX list entries, 3 words each */
#define FS_HDR 157           /* headers of the KMAX list entries, 4 words each: code, finger offset, mu, bias */
#define FS_ROW 197           /* the per-finger hand-off (DL_SSUB .. DL_CAPS) */
#define FS_HDR_HI 197        /* the headers from entry (FS_HDR_HI - FS_HDR) / 4 = 10 on, over the (then dead) hand-off */
#define FS_X 253             /* block exchange of the contact solver, 13 blocks (12 hand blocks + the box/ground block 12) x 5 quads
                                [block][quad][lane][4]: the velocity change a block made in one pass -- quad 0 = d u_B[0..3], 1 =
                                (d u_B[4], d u_B[5], d v_box[0], d v_box[1]), 2 = d v_box[2..5], 3 = d u_f of the finger of the block's
                                first contact, 4 = d u_f of the finger of its second contact when that is another one (pairs only) */
#define FS_FORCE 253         /* net contact force partial sums, 3 DEXSIM_NFSLOT words per finger wave (forces_partial) */
#define FS_T 513             /* the common velocities, 8 quads (absolute values): u_B, box twist as in FS_X, 3 + f = u_f of finger f */
#define FS_SPRE 513          /* composite part of S, lower triangle (schur_precompute) */
#define FS_SPRE_BIAS 534     /* bias of the base joints (schur_precompute) */
#define FS_BCH 545           /* axes and origins of the base joints, 9 quads (ROWADDR layout, bch_get2) */
#define FS_CTAB 581          /* work-item table, 768 entries indexed linearly: entry i = owner lane | block << 8 of the i-th hand block
                                of the workgroup (block-major: all envs' block 0, then all envs' block 1, ...) */
#define FS_NITEM 593         /* lane 0: number of items */
#define FS_CMP 594           /* lever arms r = contact point - box centre of the (at most 4) box/ground contacts, 3 words each */
#define FS_CARRY_QD 606      /* qd of the base joints, body to body (SubstepCarry) */
#define FS_CARRY_BP 612      /* box position, body to body */
#define FS_COMPCNT 615       /* lane 0: fingers whose composite + wrench are in LDS, counted over the bodies of the launch */
                             /* (word 616 is free) */
#define FS_GEN 617           /* the env's warm-start generation of this sub-step */
#define FS_SPLIT 618         /* split counts of this sub-step, packed (split_pack) */
#define FS_CPACK 619         /* corner index of box/ground list slot k in bits [3k+2 : 3k] */
#define FS_CMP_INVM 620      /* 1/m, 1/I of the box */
#define FS_FLAG 622          /* word FS_FLAG + w, w = finger 0-4 / palm 5: broadphase verdict (seq << 1) | clear in lane 0 (see
                                substep_body); then (hand clear) the Schur helpers' tokens in lane 0 (| SCHUR_SPLIT_BIT, waves 1-3) or
                                (else) the narrowphase counts of every lane (NP_*) */
#define FS_CARRY_Q 628       /* q of the base joints, body to body */
#define FS_TGTB 634          /* base DOF targets */
#define FS_WORDS 640
#define FS_LDS_BYTES (FS_WORDS * 64 * sizeof(float))

// Live phases of a region: body phases 0-5 of substep_body (0 and 1 share a bit: no barrier separates them, the box wave starts on
// phase 1 while the other waves run phase 0), the stretch between two bodies (and the prologue before the first), the publication
// behind the last body, the post block.
enum : unsigned { LIVE_ACROSS = 1u << 6, LIVE_PUB = 1u << 7, LIVE_POST = 1u << 8 };
constexpr unsigned lds_live(int first, int last) {   // body phases first .. last
  unsigned m = 0;
  for (int p = first; p <= last; p++) m |= 1u << (p == 0 ? 1 : p);
  return m;
}
constexpr unsigned LIVE_CARRY = lds_live(5, 5) | LIVE_ACROSS | lds_live(0, 0);   // phase 5 -> the next body's phase 0
constexpr unsigned LIVE_LAUNCH = lds_live(0, 5) | LIVE_ACROSS;                   // counted or seq-tagged over the bodies
struct LdsRegion { int start, words; unsigned live; };
// Waves by role: f = finger waves, palm = wave 5, box = wave 6, items = the work items of waves 0-5 (general path).
constexpr LdsRegion LDS_MAP[] = {
  // start       words                    live              written by (phase) -> read by (phase)
  {DL_SINV,      36,                      lds_live(2, 3)},  // S^-1: wave 0 (2) -> items (3); S, sum: Schur helpers, wave 0 (2) -> wave 0 (2)
  {DL_PALM,      16,                      lds_live(1, 2)},  // palm (1) -> palm (1, schur_precompute), wave 0 (2)
  {DL_NC,        1,                       lds_live(1, 5)},  // box (1), wave 0 (2) -> all (2-5)
  {FS_UB,        6,                       lds_live(2, 5)},  // wave 0 (2, or 3 without items), palm (4) -> all (5)
  {FS_BOXV,      6,                       lds_live(1, 5)},  // box (1-3), palm + box (4) -> box (3, 5)
  {FS_UF,        20,                      lds_live(1, 5)},  // f (1, 4) -> f (3, 5)
  {FS_LAM,       3 * DEXSIM_KMAX,         lds_live(1, 5)},  // box (1-4), items (3-4) -> box (1-4), items (4), f (5, forces)
  {FS_HDR,       FS_HDR_HI - FS_HDR,      lds_live(1, 5)},  // entries 0-9: box (1), items (3) -> box (1-4), items (4), f + palm (5)
  {FS_ROW,       DL_HANDOFF,              lds_live(1, 2)},  // f (1) -> palm (1), Schur phase + narrowphase (2)
  {FS_HDR_HI,    4 * DEXSIM_KMAX - (FS_HDR_HI - FS_HDR), lds_live(3, 5)},   // entries 10-23: items (3) -> items (4), f + palm (5)
  {FS_X,         13 * 5 * 4,              lds_live(3, 4)},  // all (3: zeros), items + box (4) -> reducers (4)
  {FS_FORCE,     5 * 3 * DEXSIM_NFSLOT,   lds_live(5, 5)},  // last sub-step, general path: f (5) -> f (5)
  {FS_T,         8 * 4,                   lds_live(3, 4)},  // waves 0, 6 and f (3), reducers (4) -> items, box, reducers (4)
  {FS_SPRE,      27,                      lds_live(1, 2)},  // palm (1) -> Schur phase (2)
  {FS_BCH,       36,                      lds_live(1, 3)},  // palm (1) -> items (3)
  {FS_CTAB,      12,                      lds_live(2, 4)},  // wave 0 (2) -> items (3-4)
  {FS_NITEM,     1,                       lds_live(2, 4)},  // wave 0 (2) -> all (3-4)
  {FS_CMP,       12,                      lds_live(1, 4)},  // box (1) -> box (1-4)
  {FS_CARRY_QD,  6,                       LIVE_CARRY},      // palm (5) -> waves 0-5 (0)
  {FS_CARRY_BP,  3,                       LIVE_CARRY},      // box (5) -> waves 0-5 (0)
  {FS_COMPCNT,   1,                       LIVE_LAUNCH},     // prologue (zero), f (1) -> palm (1)
  {FS_GEN,       1,                       lds_live(1, 4)},  // box (1) -> items (3), all (4)
  {FS_SPLIT,     1,                       lds_live(2, 4)},  // wave 0 (2) -> items, all (3-4)
  {FS_CPACK,     1,                       lds_live(1, 4)},  // box (1) -> box (3-4)
  {FS_CMP_INVM,  2,                       lds_live(1, 4)},  // box (1) -> box (1-4), all (4)
  {FS_FLAG,      6,                       LIVE_LAUNCH},     // prologue (zero), f + palm (0-1), helpers + narrowphase (2) -> box (1), all (2), f (4)
  {FS_CARRY_Q,   6,                       LIVE_CARRY},      // palm (5) -> waves 0-5 (0)
  {FS_TGTB,      6,                       lds_live(1, 2)},  // palm (1) -> wave 0 (2)
};
// -1 when every region of LDS_MAP and `extra` lies in [0, FS_WORDS) and no two of them live in a common phase share a word, else
// 1000 x the first word of the region at fault + the first word of the region it overlaps (+ 999: it leaves [0, FS_WORDS)).
constexpr int lds_map_conflict(LdsRegion extra = {0, 0, 0}) {
  constexpr int n = sizeof(LDS_MAP) / sizeof(LDS_MAP[0]);
  for (int i = 0; i <= n; i++) {
    const LdsRegion a = i < n ? LDS_MAP[i] : extra;
    if (a.start < 0 || a.words < 0 || a.start + a.words > FS_WORDS) return 1000 * (a.start < 0 ? 0 : a.start) + 999;
    for (int j = 0; j < i; j++) {
      const LdsRegion b = LDS_MAP[j];
      if ((a.live & b.live) && a.start < b.start + b.words && b.start < a.start + a.words) return 1000 * a.start + b.start;
    }
  }
  return -1;
}
static_assert(FS_LDS_BYTES == 160 * 1024, "the sub-step kernels own the CU's whole LDS: one workgroup per CU");
static_assert(lds_map_conflict() < 0, "LDS map: a region leaves the LDS or shares a word with a region live in a common phase "
                                      "(the note shows 1000 x the first word of one + the first word of the other)");
static_assert(DL_CAPS(0, 5) == DL_HANDOFF, "the per-finger hand-off is DL_HANDOFF words");
// the stand-alone kernels: k_dynamics' array, k_solve's dynamic LDS (u_f, impulses, headers, kstage staged contacts; solve_kstage <= 4)
#define SOLVE_LDS_WORDS(kstage) (60 + DEXSIM_KMAX * 3 + DEXSIM_KMAX * 4 + (kstage) * 3 * CROW_W)
static_assert((DL_SPLIT + 1) * 64 * sizeof(float) <= FS_LDS_BYTES, "k_dynamics' LDS does not fit into the CU's");
static_assert(SOLVE_LDS_WORDS(4) * 64 * sizeof(float) <= FS_LDS_BYTES, "k_solve's LDS does not fit into the CU's");

// finger f: everything that depends only on the base chain and the finger's own 4 joints
// state of a finger's 4 joints, loaded at kernel entry (before the base chain) so that the memory round trip
// overlaps the base-chain arithmetic instead of sitting inside the FK loop behind its jframe stores
struct FingerIn { float ql[4], qdl[4], tg[4]; };
DI void finger_load(const Arena& A, int f, int N, int e, FingerIn& in) {
#pragma unroll
  for (int l = 0; l < 4; l++) { const int j = 6 + 4 * f + l; in.ql[l] = FLD(q, j); in.qdl[l] = FLD(qd, j); in.tg[l] = FLD(targets, j); }
}

// tok_seq > 0 (fused sub-step): the finger decides itself whether it can touch anything in this sub-step (sphere_clear =
// the hand-level verdict; else the per-capsule bounds) and publishes the verdict as LDS token FS_FLAG + f; a clear finger
// skips the joint-frame / factor hand-off that only the rows of its own contacts read.  Returns the verdict.
// MS: the model structure the chain may rely on (see base_chain); false is the general form.
template <bool MS>
DI bool finger_dynamics(const Arena& A, const DevParams* __restrict__ P, const BaseChain& B, const FingerIn& in, float* sh, const int dlb,
                        float* s_uf, int lane, int f, int N, int e, int tok_seq = 0, bool sphere_clear = false,
                        V3 bpos = V3{0, 0, 0}, const M3& Rb = M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}, float* Gk = nullptr) {
  const DexHandModel& M = P->model;
  const float h = P->h;
  const int j0 = 6 + 4 * f;
  Q4 qf = B.q5; V3 of = B.o5; V3 wf = B.w5, alf = B.al5, aof = B.ao5;
  V3 a[4], o[4], cl[4], fl[4], nl[4];
  S6 Iw[4];
  float ql[4], qdl[4], tg[4];
  bool clr = true;
  if (tok_seq > 0 && sphere_clear && lane == 0) sh[(FS_FLAG + f) * 64] = __int_as_float((tok_seq << 1) | 1);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int j = j0 + l;
    ql[l] = in.ql[l]; qdl[l] = in.qdl[l]; tg[l] = in.tg[l];
    M3 Rp = q2mat(qf);
    V3 on = of + mul(Rp, v3p(P->jc[j].poff));
    Q4 qz = qmul(qf, q4p(P->jc[j].qoff));
    V3 ax = v3p(P->jc[j].axis);
    float s, c;
    sincos_joint(0.5f * ql[l], &s, &c);
    Q4 qn = qmul(qz, Q4{ax.x * s, ax.y * s, ax.z * s, c});
    M3 R = q2mat(qn);
    // (the joint's own rotation leaves its axis where the fixed offset put it: no second matrix from qz)
    // MS, flexion joints: the axis +-e_y picks a signed column of R (each product exact: never fused into a neighbour)
    V3 aw = MS && l >= 1 ? V3{mulr(R.m[1], ax.y), mulr(R.m[4], ax.y), mulr(R.m[7], ax.y)} : mul(R, ax);
    V3 r = on - of;
    V3 aoj = aof + cross(alf, r) + cross(wf, cross(wf, r));
    V3 cw = cross(wf, aw);
    alf += qdl[l] * cw; wf += qdl[l] * aw; aof = aoj;
    cl[l] = on + mul(R, v3p(P->jc[j].com));
    // link inertias diagonal in their joint frames (a host-side check of the whole model, DevParams::inertia_diag): R diag R^T in 27
    // instead of 45 multiply-adds -- a uniform branch, fused sub-step only (tok_seq > 0 is a compile-time constant after inlining:
    // in the un-fused test kernel the second code path cost 100 B of scratch).  63.3 -> 63.9 M env-steps/s, two A/B pairs on one box.
    Iw[l] = (tok_seq > 0 && P->inertia_diag) ? rotate_inertia_diag(R, P->jc[j].inertia) : rotate_inertia(R, P->jc[j].inertia);
    V3 rc = cl[l] - on;
    V3 ac = aof + cross(alf, rc) + cross(wf, cross(wf, rc));
    fl[l] = P->jc[j].mass * ac;
    nl[l] = mul(Iw[l], alf) + cross(wf, mul(Iw[l], wf)) + cross(rc, fl[l]);
    if (l >= 1 && !(tok_seq > 0 && sphere_clear)) {
      const int cap = 3 + 3 * f + (l - 1);
      const V3 c0 = on + mul(R, v3p(M.cap_p0[cap])), c1 = on + mul(R, v3p(M.cap_p1[cap]));
      sh_put3(sh, lane, DL_CAPS(dlb, f) + 6 * (l - 1), c0);
      sh_put3(sh, lane, DL_CAPS(dlb, f) + 6 * (l - 1) + 3, c1);
      if (tok_seq > 0) clr = clr && capsule_clear(c0, c1, M.cap_r[cap], P->cfg, bpos, Rb);
    }
    a[l] = aw; o[l] = on; qf = qn; of = on;
  }
  bool fclear = false;
  if (tok_seq > 0) {
    fclear = sphere_clear || __all(clr);
    if (!sphere_clear && lane == 0) sh[(FS_FLAG + f) * 64] = __int_as_float((tok_seq << 1) | (fclear ? 1 : 0));
  }
  if (!fclear) {   // joint frames: read only by the rows of this finger's contacts
    const float w24[24] = {a[0].x, a[0].y, a[0].z, o[0].x, o[0].y, o[0].z, a[1].x, a[1].y, a[1].z, o[1].x, o[1].y, o[1].z,
                           a[2].x, a[2].y, a[2].z, o[2].x, o[2].y, o[2].z, a[3].x, a[3].y, a[3].z, o[3].x, o[3].y, o[3].z};
#pragma unroll
    for (int qd = 0; qd < 6; qd++) *FQ(jframe, JFRAME_FQ0 + 6 * f + qd) = f4{w24[4 * qd], w24[4 * qd + 1], w24[4 * qd + 2], w24[4 * qd + 3]};
  }
  // RNEA backward: joint bias + the finger's wrench about o5
  float bias[4];
#pragma unroll
  for (int l = 3; l >= 0; l--) {
    bias[l] = dot(a[l], nl[l]);
    if (l > 0) { fl[l - 1] += fl[l]; nl[l - 1] += nl[l] + cross(o[l] - o[l - 1], fl[l]); }
  }
  sh_put3(sh, lane, DL_WRENCH(dlb, f), fl[0]);
  sh_put3(sh, lane, DL_WRENCH(dlb, f) + 3, nl[0] + cross(o[0] - B.o5, fl[0]));
  // CRBA blocks from the composite bodies of the finger
  float Fm[16], Cm[24]; // Cm[i*4 + l]
  Comp cc;
#pragma unroll
  for (int l = 3; l >= 0; l--) {
    Comp b; b.m = P->jc[j0 + l].mass; b.c = cl[l]; b.I = Iw[l];
    if (l == 3) cc = b; else { comp_add(b, cc); cc = b; }
    V3 Pm = cc.m * cross(a[l], cc.c - o[l]);
    V3 Lm = mul(cc.I, a[l]);
#pragma unroll
    for (int k = 0; k <= l; k++) {
      float v = dot(a[k], Lm + cross(cc.c - o[k], Pm));
      Fm[l * 4 + k] = v; Fm[k * 4 + l] = v;
    }
    if (MS) {   // prismatic axes e_x, e_y, e_z: a component each; joint frames 3-5 share their origin: one lever-arm product
      const V3 Xm = Lm + cross(cc.c - B.ob[3], Pm);
      Cm[l] = Pm.x; Cm[4 + l] = Pm.y; Cm[8 + l] = Pm.z;
#pragma unroll
      for (int i = 3; i < 6; i++) Cm[i * 4 + l] = dot(B.ab[i], Xm);
    } else {
#pragma unroll
      for (int i = 0; i < 6; i++)
        Cm[i * 4 + l] = i < 3 ? dot(B.ab[i], Pm) : dot(B.ab[i], Lm + cross(cc.c - B.ob[i], Pm));
    }
  }
  comp_put(sh, lane, DL_COMP(dlb, f), cc, B.o5);
  if (tok_seq > 0) {   // composite + wrench are in LDS: count this finger in for the palm wave's schur_precompute
    asm volatile("" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add((int*)(sh + FS_COMPCNT * 64), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  float tau[4];
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int j = j0 + l;
    const float kp = P->jc[j].kp, kdh = P->jc[j].kd + h * kp;
    Fm[l * 4 + l] += P->jc[j].armature + h * kdh;
    tau[l] = kp * (tg[l] - ql[l]) - kdh * qdl[l] - bias[l];
  }
  spd_inverse<4>(Fm); // Fm := Fhat_f^-1
  float G[24];        // G[l*6 + i]
  // the 6-wide products (G_f, C_f G_f, G_f^T tau) in packed FP32, two neighbouring base-joint columns per instruction (v_pk_fma_f32;
  // each component is the same fused multiply-add chain as the one-column form)
  f2 G2[12];          // G2[l*3 + ip] = (G[l*6 + 2 ip], G[l*6 + 2 ip + 1])
#pragma unroll
  for (int l = 0; l < 4; l++)
#pragma unroll
    for (int ip = 0; ip < 3; ip++) {
      f2 s2 = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; k++) s2 = f2{Cm[(2 * ip) * 4 + k], Cm[(2 * ip + 1) * 4 + k]} * Fm[l * 4 + k] + s2;
      G2[l * 3 + ip] = s2;
      G[l * 6 + 2 * ip] = s2.x; G[l * 6 + 2 * ip + 1] = s2.y;
    }
  // G_f: the rows of the finger's contacts read it (other lanes, phase 3) and this wave itself needs it again in phase 5.  With the
  // whole hand clear of box and ground (hand-level bound, uniform over the workgroup: the sub-step takes the hand-clear path for
  // certain) it stays in registers (Gk) for the two short phases in between and is NOT written: 480 B per env and sub-step, the
  // largest single item of the step kernel's write traffic, and the L2 round trip at the head of phase 5.
  if (!(tok_seq > 0 && sphere_clear && Gk)) {
#pragma unroll
    for (int qd = 0; qd < 6; qd++) *FQ(fac_g, 6 * f + qd) = f4{G[4 * qd], G[4 * qd + 1], G[4 * qd + 2], G[4 * qd + 3]};
  }
  if (Gk) {
#pragma unroll
    for (int i = 0; i < 24; i++) Gk[i] = G[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int kp = 0; kp <= i / 2; kp++) {
      f2 s2 = {0.f, 0.f};
#pragma unroll
      for (int l = 0; l < 4; l++) s2 = G2[l * 3 + kp] * Cm[i * 4 + l] + s2;
      SH(DL_SSUB(dlb, f) + i * (i + 1) / 2 + 2 * kp) = s2.x;
      if (2 * kp + 1 <= i) SH(DL_SSUB(dlb, f) + i * (i + 1) / 2 + 2 * kp + 1) = s2.y;
    }
  if (!fclear) {   // lower triangle, row by row: 10 words in 3 quads
    *FQ(fac_finv, 3 * f) = f4{Fm[0], Fm[4], Fm[5], Fm[8]};
    *FQ(fac_finv, 3 * f + 1) = f4{Fm[9], Fm[10], Fm[12], Fm[13]};
    *FQ(fac_finv, 3 * f + 2) = f4{Fm[14], Fm[15], 0.f, 0.f};
  }
#pragma unroll
  for (int ip = 0; ip < 3; ip++) {
    f2 s2 = {0.f, 0.f};
#pragma unroll
    for (int l = 0; l < 4; l++) s2 = G2[l * 3 + ip] * tau[l] + s2;
    SH(DL_GSUM(dlb, f) + 2 * ip) = s2.x; SH(DL_GSUM(dlb, f) + 2 * ip + 1) = s2.y;
  }
#pragma unroll
  for (int l = 0; l < 4; l++) {
    float s = qdl[l];
#pragma unroll
    for (int i = 0; i < 6; i++) s += G[l * 6 + i] * B.qdb[i];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) acc += Fm[l * 4 + k] * tau[k];
    const float uf = s + h * acc;
    if (s_uf) s_uf[(4 * f + l) * 64 + lane] = uf;   // fused sub-step: hand the free velocity to the solver through LDS
    else FLD(ufree, j0 + l) = uf;
  }
  return fclear;
}

// base block: B from the total composite, Schur complement, tau_B, u_B.  Runs on wave 0 after the hand-off.
// solve_only (fused sub-step without hand contacts): only u_B is needed -- Cholesky solve instead of the full inverse, and
// S^-1 is neither formed nor handed on through LDS (the contact rows of the general path are its only readers).
// SCHUR_SPLIT (fused sub-step, hand clear): the Schur phase is the one serial stretch of a sub-step -- wave 0 alone while five
// waves wait at the barrier.  It is cut twice.  (1) Everything that depends on the composites and wrenches only -- the
// composite part of the 21 entries of S, the bias of the six base joints -- is formed by the palm wave during phase 1
// (schur_precompute: the fingers' composites are in LDS half-way through their phase 1, the palm wave is idle from then on).
// (2) Behind the barrier three waves take the finger sums that do not depend on one another: job 0 (wave 1) = row 3 and the last
// two entries of row 5 of S, job 2 (wave 3) = row 4, job 1 (wave 2) = the sum of G_f^T tau_f and rows 0-2; wave 0 keeps the first
// four entries of row 5, the PD terms and the Cholesky solve.  Same expressions and accumulation order as the unsplit
// schur_base; results in the (then unused) S^-1 words (21 + 12), hand-over by the job's token (FS_FLAG + job wave, bit 30 =
// "posted").  (Round 2 had the helpers form the composite part too, each from its own copy of the composite sum: ~100 LDS words
// per lane and helper; round 3 moved it into phase 1: Schur phase 6.0k -> 4.4k cycles.)
#define SCHUR_SPLIT_BIT (1 << 30)
// The LDS token waits (here and in the box wave's phase 1) are safe because all seven waves of a workgroup are co-resident and
// the waves waited for never wait for the waiter first.  A sequencing bug in a later edit would turn them into a GPU hang.  The
// diagnostic build -DDEXSIM_DEBUG_SPIN=<bound> (tests/test_gpu_parity.py::test_debug_spin_build...) bounds every wait: after
// <bound> polls it records (site << 24 | seq) in counters[CNT_SPIN_TIMEOUT] and falls through, so the launch always drains and the
// test fails on the recorded word instead of hanging the box.  The product build compiles the guards away.
#ifdef DEXSIM_DEBUG_SPIN
#define SPIN_GUARD_INIT() int spin_polls_ = 0
#define SPIN_GUARD(cntp, site, seq) if (++spin_polls_ > (DEXSIM_DEBUG_SPIN)) { if (cntp) GPTR(cntp)[CNT_SPIN_TIMEOUT] = ((site) << 24) | (seq); break; }
#else
#define SPIN_GUARD_INIT() do {} while (0)
#define SPIN_GUARD(cntp, site, seq) do {} while (0)
#endif
DI Comp schur_comp(const float* sh, const int dlb, int lane, V3 o5) {
  float M = SH(DL_PALM);
  V3 sd = M * sh_get3(sh, lane, DL_PALM + 1);
  S6 J = {SH(DL_PALM + 4), SH(DL_PALM + 5), SH(DL_PALM + 6), SH(DL_PALM + 7), SH(DL_PALM + 8), SH(DL_PALM + 9)};
#pragma unroll
  for (int f = 0; f < 5; f++) {
    const float mf = SH(DL_COMP(dlb, f));
    M += mf;
    sd += mf * sh_get3(sh, lane, DL_COMP(dlb, f) + 1);
    J = J + S6{SH(DL_COMP(dlb, f) + 4), SH(DL_COMP(dlb, f) + 5), SH(DL_COMP(dlb, f) + 6), SH(DL_COMP(dlb, f) + 7), SH(DL_COMP(dlb, f) + 8), SH(DL_COMP(dlb, f) + 9)};
  }
  // (operator, not rcp_n, although M is a sum of link masses: this reciprocal -- like five of the block sweeps' split factors 1/n --
  // is the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence in this build, not the scaled v_rcp_f32, and a helper
  // would change its last bit)
  const float inv = M > 0.f ? 1.f / M : 0.f;
  const V3 d = inv * sd;
  const S6 sh_back = pa(M, d);
  Comp c;
  c.m = M; c.c = o5 + d;
  c.I = {J.xx - sh_back.xx, J.yy - sh_back.yy, J.zz - sh_back.zz, J.xy - sh_back.xy, J.xz - sh_back.xz, J.yz - sh_back.yz};
  return c;
}
// row i of S (entries k0 .. k1 <= i) in the split Schur phase: the composite part (schur_precompute) minus the fingers' C_f G_f,
// summed finger by finger
template <int i, int k0 = 0, int k1 = i>
DI void schur_row(float* sh, const int dlb, int lane) {
  float r[k1 - k0 + 1];
#pragma unroll
  for (int k = k0; k <= k1; k++) {
    const float v = SH(FS_SPRE + i * (i + 1) / 2 + k);
    float ss = 0.f;
#pragma unroll
    for (int f = 0; f < 5; f++) ss += SH(DL_SSUB(dlb, f) + i * (i + 1) / 2 + k);
    r[k - k0] = v - ss;
  }
#pragma unroll
  for (int k = k0; k <= k1; k++) SH(DL_SCHUR_S + i * (i + 1) / 2 + k) = r[k - k0];
}
// The composite part of S (the 21 entries before the fingers' C_f G_f are subtracted) and the bias of the six base joints
// depend on the fingers' composites and wrenches only, which are in LDS half-way through phase 1: the palm wave, idle from
// then on, forms them (same expressions and order as the unsplit schur_base) and leaves them in
// FS_SPRE; the Schur phase behind the barrier then only subtracts the finger sums.  The fingers count themselves in at
// FS_COMPCNT (5 per body of a launch).
DI void schur_precompute(float* sh, const int dlb, int lane, const BaseChain& B, int seq, int* dbg_cnt) {
  {
    SPIN_GUARD_INIT();
    while (lds_cnt_load(sh, FS_COMPCNT * 64) < 5 * seq) { __builtin_amdgcn_s_sleep(2); SPIN_GUARD(dbg_cnt, 4, seq); }
  }
  asm volatile("" ::: "memory");
  const Comp comp5 = schur_comp(sh, dlb, lane, B.o5);
  int idx = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    V3 Pm, Lm;
    if (i < 3) { Pm = comp5.m * B.ab[i]; Lm = {0, 0, 0}; }
    else { Pm = comp5.m * cross(B.ab[i], comp5.c - B.ob[i]); Lm = mul(comp5.I, B.ab[i]); }
#pragma unroll
    for (int k = 0; k <= i; k++) {
      SH(FS_SPRE + idx) = k < 3 ? dot(B.ab[k], Pm) : dot(B.ab[k], Lm + cross(comp5.c - B.ob[k], Pm));
      idx++;
    }
  }
  V3 ff = sh_get3(sh, lane, DL_PALM_WRENCH), nn = sh_get3(sh, lane, DL_PALM_WRENCH + 3);
#pragma unroll
  for (int f = 0; f < 5; f++) {
    ff += sh_get3(sh, lane, DL_WRENCH(dlb, f));
    nn += sh_get3(sh, lane, DL_WRENCH(dlb, f) + 3);
  }
  SH(FS_SPRE_BIAS + 5) = dot(B.ab[5], nn);
#pragma unroll
  for (int j = 4; j >= 0; j--) {
    nn += cross(B.ob[j + 1] - B.ob[j], ff);
    SH(FS_SPRE_BIAS + j) = j < 3 ? dot(B.ab[j], ff) : dot(B.ab[j], nn);
  }
}
DI void schur_helper(float* sh, const int dlb, int job, int lane) {
  if (job == 1) {
    float gsum[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < 5; f++)
#pragma unroll
      for (int i = 0; i < 6; i++) gsum[i] += SH(DL_GSUM(dlb, f) + i);
#pragma unroll
    for (int i = 0; i < 6; i++) SH(DL_SCHUR_GSUM + i) = gsum[i];
    schur_row<0>(sh, dlb, lane); schur_row<1>(sh, dlb, lane); schur_row<2>(sh, dlb, lane);
  } else if (job == 0) {
    schur_row<3>(sh, dlb, lane); schur_row<5, 4, 5>(sh, dlb, lane);
  } else schur_row<4>(sh, dlb, lane);
}

// split_seq > 0 (fused sub-step, hand clear): the finger sums come from schur_helper on two other waves; this wave forms the
// composite part of S meanwhile and picks the sums up behind their tokens.
DI void schur_base(const Arena& A, const DevParams* __restrict__ P, const BaseChain& B, float* sh, const int dlb, float* uB_out,
                   int lane, int N, int e, int tgt_lds = -1, bool solve_only = false, int split_seq = 0,
                   const Stamps st = {}, int* dbg_cnt = nullptr) {
  const float h = P->h;
  st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_START);
  Comp comp5;
  V3 f5 = sh_get3(sh, lane, DL_PALM_WRENCH), n5 = sh_get3(sh, lane, DL_PALM_WRENCH + 3);
  float Ssub[21], gsum[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 21; i++) Ssub[i] = 0.f;
  if (split_seq == 0) comp5 = schur_comp(sh, dlb, lane, B.o5);   // (split: the composite part comes from schur_precompute)
  if (split_seq == 0) {
#pragma unroll
    for (int f = 0; f < 5; f++) {   // (unrolled: the five fingers' LDS reads are in flight together; rolled, every iteration
                                    // waited for its own)
      f5 += sh_get3(sh, lane, DL_WRENCH(dlb, f));
      n5 += sh_get3(sh, lane, DL_WRENCH(dlb, f) + 3);
#pragma unroll
      for (int i = 0; i < 21; i++) Ssub[i] += SH(DL_SSUB(dlb, f) + i);
#pragma unroll
      for (int i = 0; i < 6; i++) gsum[i] += SH(DL_GSUM(dlb, f) + i);
    }
  }
  st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_COMPOSITE);   // composite sum done
  float S[36];
  if (split_seq > 0) schur_row<5, 0, 3>(sh, dlb, lane);   // (the other rows come from the helpers)
  else {
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      V3 Pm, Lm;
      if (i < 3) { Pm = comp5.m * B.ab[i]; Lm = {0, 0, 0}; }
      else { Pm = comp5.m * cross(B.ab[i], comp5.c - B.ob[i]); Lm = mul(comp5.I, B.ab[i]); }
#pragma unroll
      for (int k = 0; k <= i; k++) {
        float v = k < 3 ? dot(B.ab[k], Pm) : dot(B.ab[k], Lm + cross(comp5.c - B.ob[k], Pm));
        v -= Ssub[idx++];
        S[i * 6 + k] = v; S[k * 6 + i] = v;
      }
    }
  }
  st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_OWN_ROWS);   // own rows done
  // The PD terms of the base joints need none of the finger sums: they stand in front of the wait for the helpers' tokens, so that
  // the scalar loads of kp / kd / armature and the reads of the staged targets are in flight while the helpers finish (behind the
  // wait they were issued only once the tokens had arrived).  Same expressions and association as when they stood at "S, tau_B".
  float dgn[6];    // armature + h kdh: what the PD controller adds to the diagonal of S
  float tauB[6];   // here the PD part kp (tgt - q) - kdh qd; "- bias - gsum" follows below
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const float kp = P->jc[i].kp, kdh = P->jc[i].kd + h * kp;
    dgn[i] = P->jc[i].armature + h * kdh;
    // fused sub-step: the base targets were staged in LDS by wave 5 (a global load here would first have to wait for
    // this wave's own factor stores of phase 1 to drain)
    const float tgt = tgt_lds >= 0 ? SH(tgt_lds + i) : FLD(targets, i);
    tauB[i] = kp * (tgt - B.qb[i]) - kdh * B.qdb[i];
  }
  float bias[6];
  if (split_seq > 0) {
    // (the values above exist before the first poll: the optimiser may not sink them behind the loop)
    asm volatile("" :: "v"(dgn[0]), "v"(dgn[1]), "v"(dgn[2]), "v"(dgn[3]), "v"(dgn[4]), "v"(dgn[5]),
                 "v"(tauB[0]), "v"(tauB[1]), "v"(tauB[2]), "v"(tauB[3]), "v"(tauB[4]), "v"(tauB[5]));
    // pick up the helpers' sums (DS instructions of a wave execute in order: data stores, then the token store; here the token
    // load, then the data loads -- only the compiler has to be kept from reordering them).  One read per poll: lane l < 3 reads
    // the token of helper wave 1 + l, the other lanes read wave 1's again, and the vote passes once all three are posted.
    const int want = (split_seq << 1) | 1 | SCHUR_SPLIT_BIT;
    const int tw = (FS_FLAG + 1 + (lane < 3 ? lane : 0)) * 64;
    {
      SPIN_GUARD_INIT();
      while (!__all(lds_tok_load(sh, tw) == want)) { __builtin_amdgcn_s_sleep(1); SPIN_GUARD(dbg_cnt, 1, split_seq); }
    }
    asm volatile("" ::: "memory");
    st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_TOKENS);   // tokens seen
    {
      int idx = 0;
#pragma unroll
      for (int i = 0; i < 6; i++)
#pragma unroll
        for (int k = 0; k <= i; k++) {
          const float v = SH(DL_SCHUR_S + idx); idx++;
          S[i * 6 + k] = v; S[k * 6 + i] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) { bias[i] = SH(FS_SPRE_BIAS + i); gsum[i] = SH(DL_SCHUR_GSUM + i); }
  } else {
    V3 nn = n5, ff = f5;
    bias[5] = dot(B.ab[5], nn);
#pragma unroll
    for (int j = 4; j >= 0; j--) {
      nn += cross(B.ob[j + 1] - B.ob[j], ff);
      bias[j] = j < 3 ? dot(B.ab[j], ff) : dot(B.ab[j], nn);
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    S[i * 6 + i] += dgn[i];
    tauB[i] = tauB[i] - bias[i] - gsum[i];
  }
  st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_S_TAUB);   // S, tau_B complete
  if (solve_only) {
    float x[6];
    spd_solve<6>(S, tauB, x);
#pragma unroll
    for (int i = 0; i < 6; i++) uB_out[i] = B.qdb[i] + h * x[i];
    st.mark<SG_SCHUR>(A, N, 0, e, SCHUR_SOLVED);   // solved
    return;
  }
  spd_inverse<6>(S);
  // S^-1 for the contact rows: 9 quads [quad][lane][4] (ROWADDR layout) -- the row builder reads two rows of S^-1 with three
  // 16-byte LDS reads (round 2: 36 words [word][lane], 36 reads per contact)
#pragma unroll
  for (int qd = 0; qd < 9; qd++) *(f4*)(sh + DL_SINV * 64 + ROWADDR(4 * qd, lane)) = f4{S[4 * qd], S[4 * qd + 1], S[4 * qd + 2], S[4 * qd + 3]};
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) acc += S[i * 6 + k] * tauB[k];
    const float ub = B.qdb[i] + h * acc;
    if (uB_out) uB_out[i] = ub;
    else FLD(ufree, i) = ub;
  }
}

// rows of contact k in u-space: t = j_B - G_f^T j_f, S^-1 t, Fhat_f^-1 j_f, box parts, 1/D, bias
// FUSED (k_physics4 / k_physics1, general path): the rows go to the arena in the quad layout of the LDS row store (crowq:
// [quad][env][4], so that a 16-byte access moves four row words of a lane), header and starting impulses to LDS (FS_HDR, FS_LAM),
// and the base joints' axes and origins come from LDS (FS_BCH; B = nullptr).
// !FUSED (stand-alone k_dynamics): SoA arena rows (crow), header and starting impulses to the arena (chdr, clam) for k_solve, base
// joints from B.
// split: the env's packed split counts (SPLIT_*; 0 = no splitting): 1/D and the in-contact couplings A_rs are those of the contact
// inside its solver block, where the hand base, the contact's finger and the box respond nB, nF and nX times as strongly.
// gen >= 0: warm start -- the contact's starting impulses come from the cache (slot by capsule / type / sample, valid while its
// tag is 8 * gen); gen < 0: they start at zero.
template <bool FUSED>
DI void build_contact_rows(const Arena& A, const DevParams* __restrict__ P, const BaseChain* B, float* sh, int lane, int k, int N, int e,
                           int split, int gen) {
  // Built matrix by matrix, not row by row: every operand matrix (base joint frames, finger joint frames, G_f, Fhat_f^-1, S^-1)
  // is consumed for all three rows as soon as it is used, so that at most one of them is live next to the ~80 output words.
  // (Round 2 first looped over the rows with all five matrices live -- ~200 values: inlined in the sub-step kernel that cost
  // VGPR spills, and ANY scratch use makes short bursts of launches ~1.5x slower on this part, see DESIGN.md section 3.)
  const DexSimConfig& C = P->cfg;
  const float h = P->h;
  // ---- loads, round 1: the manifold entry, the box
  const f4 cg0 = *FQ(cgeom, 2 * k), cg1 = *FQ(cgeom, 2 * k + 1);
  const V3 p = {cg0.x, cg0.y, cg0.z};
  const V3 n = {cg0.w, cg1.x, cg1.y};
  const float gap = cg1.z, mu_k = cg1.w;
  const int code = FLD(ccode, k), type = CODE_TYPE(code);
  float inv_m = 0.f, inv_I = 0.f;
  V3 bpos = {0, 0, 0};
  if (C.has_box) {
    if (!C.box_fixed) { inv_m = rcp_n(FLD(box_mass, 0)); inv_I = P->box_inv_I_k * inv_m; }   // (static box: 1/m = 1/I = 0)  [rcp_n: a body mass in kg]
    bpos = {FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2)};
  }
  const int f = type != 2 ? CODE_FINGER(code) : -1, lvl = f >= 0 ? CODE_LEVEL(code) : -1;   // (looked up by the narrowphase)
  const int nFi = (split && f >= 0) ? SPLIT_NF(split, f) : 1;
  const float nB = split ? (float)SPLIT_NB(split) : 1.f, nX = split ? (float)SPLIT_NX(split) : 1.f, nF = (float)nFi;
  // ---- loads, round 2 (they depend on the code): finger joint frames, G_f, Fhat_f^-1, the warm-start cache slot
  // (box/ground contacts -- stand-alone k_dynamics only -- are cached by list slot, with the corner in the tag)
  f4 wq = {0.f, 0.f, 0.f, 0.f};
  if (gen >= 0) wq = *(const __attribute__((address_space(1))) f4*)(A.wlam + ((size_t)(type == 2 ? 80 + k : CODE_HKEY(code)) * N + e) * 4);
  float jfr[24], G[24], Fi[10];
  if (f >= 0) {   // 15 quad loads (f differs from lane to lane: 32-bit lane offsets from the fields' scalar bases)
    const unsigned qs = (unsigned)N * 16u, oe = (unsigned)e * 16u;
    const unsigned oj = (unsigned)(JFRAME_FQ0 + 6 * f) * qs + oe, og = (unsigned)(6 * f) * qs + oe, of = (unsigned)(3 * f) * qs + oe;
    f4 qj[6], qg[6], qf[3];
#pragma unroll
    for (int qd = 0; qd < 6; qd++) {
      qj[qd] = *(const __attribute__((address_space(1))) f4*)((const char*)A.jframe + (oj + (unsigned)qd * qs));
      qg[qd] = *(const __attribute__((address_space(1))) f4*)((const char*)A.fac_g + (og + (unsigned)qd * qs));
    }
#pragma unroll
    for (int qd = 0; qd < 3; qd++) qf[qd] = *(const __attribute__((address_space(1))) f4*)((const char*)A.fac_finv + (of + (unsigned)qd * qs));
#pragma unroll
    for (int qd = 0; qd < 6; qd++) {
      jfr[4 * qd] = qj[qd].x; jfr[4 * qd + 1] = qj[qd].y; jfr[4 * qd + 2] = qj[qd].z; jfr[4 * qd + 3] = qj[qd].w;
      G[4 * qd] = qg[qd].x; G[4 * qd + 1] = qg[qd].y; G[4 * qd + 2] = qg[qd].z; G[4 * qd + 3] = qg[qd].w;
    }
    Fi[0] = qf[0].x; Fi[1] = qf[0].y; Fi[2] = qf[0].z; Fi[3] = qf[0].w; Fi[4] = qf[1].x; Fi[5] = qf[1].y; Fi[6] = qf[1].z; Fi[7] = qf[1].w;
    Fi[8] = qf[2].x; Fi[9] = qf[2].y;
  }
  const bool lim = type == 3;   // joint-limit row: J = +-e_j on one finger joint, rows 1 and 2 empty
  V3 dir[3];
  dir[0] = n;
  tangent_basis(lim ? v3(0, 0, 1) : n, dir[1], dir[2]);
  if (lim) { dir[1] = v3(0, 0, 0); dir[2] = v3(0, 0, 0); }   // (n = 0 already)
  float t[3][6], jf[3][4], St[3][6], Fj[3][4];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int i = 0; i < 6; i++) { t[r][i] = 0.f; St[r][i] = 0.f; }
#pragma unroll
    for (int l = 0; l < 4; l++) { jf[r][l] = 0.f; Fj[r][l] = 0.f; }
  }
  float Dq[3] = {0.f, 0.f, 0.f};   // J_r Mhat_block^-1 J_r^T, split-scaled
  float A10 = 0.f, A20 = 0.f, A21 = 0.f;
  if (type != 2) {
    // (1) hand base: t_r[i] = d_r . c_i, c_i = axis (prismatic) / axis x (p - origin) (revolute) of base joint i
#pragma unroll
    for (int i2 = 0; i2 < 3; i2++) {
      V3 aa[2], oo[2];
      if (FUSED) {   // two joints = 3 quads (bch_get2)
        bch_get2(sh + FS_BCH * 64, lane, i2, aa[0], oo[0], aa[1], oo[1]);
      } else { aa[0] = B->ab[2 * i2]; oo[0] = B->ob[2 * i2]; aa[1] = B->ab[2 * i2 + 1]; oo[1] = B->ob[2 * i2 + 1]; }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int i = 2 * i2 + h;
        const V3 ci = i < 3 ? aa[h] : cross(aa[h], p - oo[h]);
#pragma unroll
        for (int r = 0; r < 3; r++) t[r][i] = dot(dir[r], ci);
      }
    }
    if (f >= 0) {
      // (2) finger joints up to the capsule's level: jf_r[l] = d_r . (axis_l x (p - origin_l))
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const V3 al = {jfr[6 * l], jfr[6 * l + 1], jfr[6 * l + 2]}, ol = {jfr[6 * l + 3], jfr[6 * l + 4], jfr[6 * l + 5]};
        const V3 cl = cross(al, p - ol);
#pragma unroll
        for (int r = 0; r < 3; r++) jf[r][l] = l <= lvl ? dot(dir[r], cl) : 0.f;
        if (lim) jf[0][l] = l == lvl ? (CODE_SAMPLE(code) ? -1.f : 1.f) : 0.f;
      }
      // (3) decoupled coordinates: t_r -= G_f^T jf_r
#pragma unroll
      for (int l = 0; l < 4; l++)
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int r = 0; r < 3; r++) t[r][i] -= G[l * 6 + i] * jf[r][l];
      // (4) Fj_r = Fhat_f^-1 jf_r (symmetric 4 x 4, lower triangle packed row by row)
#pragma unroll
      for (int l = 0; l < 4; l++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const float fv = Fi[l >= kk ? l * (l + 1) / 2 + kk : kk * (kk + 1) / 2 + l];
#pragma unroll
          for (int r = 0; r < 3; r++) Fj[r][l] += fv * jf[r][kk];
        }
#pragma unroll
      for (int r = 0; r < 3; r++) {
        float s = 0.f;
#pragma unroll
        for (int l = 0; l < 4; l++) s += jf[r][l] * Fj[r][l];
        Dq[r] += nF * s;
      }
      A10 += nF * (jf[1][0] * Fj[0][0] + jf[1][1] * Fj[0][1] + jf[1][2] * Fj[0][2] + jf[1][3] * Fj[0][3]);
      A20 += nF * (jf[2][0] * Fj[0][0] + jf[2][1] * Fj[0][1] + jf[2][2] * Fj[0][2] + jf[2][3] * Fj[0][3]);
      A21 += nF * (jf[2][0] * Fj[1][0] + jf[2][1] * Fj[1][1] + jf[2][2] * Fj[1][2] + jf[2][3] * Fj[1][3]);
    }
    // (5) St_r = S^-1 t_r, two rows of S^-1 (12 words = 3 quads) at a time from LDS
#pragma unroll
    for (int i2 = 0; i2 < 3; i2++) {
      const f4 s0 = *(const f4*)(sh + DL_SINV * 64 + ROWADDR(12 * i2, lane)), s1 = *(const f4*)(sh + DL_SINV * 64 + ROWADDR(12 * i2 + 4, lane)),
               s2 = *(const f4*)(sh + DL_SINV * 64 + ROWADDR(12 * i2 + 8, lane));
      const float si[12] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w};
#pragma unroll
      for (int h = 0; h < 2; h++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
          float s = 0.f;
#pragma unroll
          for (int kk = 0; kk < 6; kk++) s += si[6 * h + kk] * t[r][kk];
          St[r][2 * i2 + h] = s;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 6; i++) s += t[r][i] * St[r][i];
      Dq[r] += nB * s;
    }
    {
      float s10 = 0.f, s20 = 0.f, s21 = 0.f;
#pragma unroll
      for (int i = 0; i < 6; i++) { s10 += t[1][i] * St[0][i]; s20 += t[2][i] * St[0][i]; s21 += t[2][i] * St[1][i]; }
      A10 += nB * s10; A20 += nB * s20; A21 += nB * s21;
    }
  }
  // (6) box part: -(d_r, rb x d_r) for hand/box contacts, +(d_r, rb x d_r) for box/ground contacts
  V3 db[3], rxd[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { db[r] = {0, 0, 0}; rxd[r] = {0, 0, 0}; }
  if (type == 1 || type == 2) {
    const float sgn = type == 2 ? 1.f : -1.f;
    const V3 rb = p - bpos;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const V3 c = cross(rb, dir[r]);
      db[r] = sgn * dir[r]; rxd[r] = sgn * c;
      Dq[r] += nX * (inv_m + inv_I * dot(c, c));
    }
    const float xm = nX * inv_m, xI = nX * inv_I;
    A10 += xm * dot(db[1], db[0]) + xI * dot(rxd[1], rxd[0]);
    A20 += xm * dot(db[2], db[0]) + xI * dot(rxd[2], rxd[0]);
    A21 += xm * dot(db[2], db[1]) + xI * dot(rxd[2], rxd[1]);
  }
  // ---- output: 3 rows x 28 words (t6 jf4 St6 Fj4 d3 rxd3 1/D pad); pad of rows 0, 1, 2 = A10, A20, A21 (A_rs = J_r Mhat^-1 J_s^T:
  // lets the solver take a contact's three J.u products against the velocities at contact entry)
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float Dinv = (lim && r > 0) ? 0.f : 1.f / (Dq[r] + 1e-9f);   // (operator: see the note at the box block's 1/D)
    const float pad = r == 0 ? A10 : (r == 1 ? A20 : A21);
    const int rw = (k * 3 + r) * CROW_W;
    if (FUSED) {   // quad layout in the arena
      float* qb = A.crowq + ((size_t)(k * 21 + r * 7) * N + e) * 4;
      st4_global(qb, t[r][0], t[r][1], t[r][2], t[r][3]);
      st4_global(qb + (size_t)1 * N * 4, t[r][4], t[r][5], jf[r][0], jf[r][1]);
      st4_global(qb + (size_t)2 * N * 4, jf[r][2], jf[r][3], St[r][0], St[r][1]);
      st4_global(qb + (size_t)3 * N * 4, St[r][2], St[r][3], St[r][4], St[r][5]);
      st4_global(qb + (size_t)4 * N * 4, Fj[r][0], Fj[r][1], Fj[r][2], Fj[r][3]);
      st4_global(qb + (size_t)5 * N * 4, db[r].x, db[r].y, db[r].z, rxd[r].x);
      st4_global(qb + (size_t)6 * N * 4, rxd[r].y, rxd[r].z, Dinv, pad);
    } else {   // stand-alone kernels: rows go through the SoA arena rows
#pragma unroll
      for (int i = 0; i < 6; i++) { FLD(crow, rw + i) = t[r][i]; FLD(crow, rw + 10 + i) = St[r][i]; }
#pragma unroll
      for (int l = 0; l < 4; l++) { FLD(crow, rw + 6 + l) = jf[r][l]; FLD(crow, rw + 16 + l) = Fj[r][l]; }
      FLD(crow, rw + 20) = db[r].x; FLD(crow, rw + 21) = db[r].y; FLD(crow, rw + 22) = db[r].z;
      FLD(crow, rw + 23) = rxd[r].x; FLD(crow, rw + 24) = rxd[r].y; FLD(crow, rw + 25) = rxd[r].z;
      FLD(crow, rw + 26) = Dinv; FLD(crow, rw + 27) = pad;
    }
  }
  // h: the sub-step, 1e-4 .. 1e-1 s; the gap is zero or a rounding residue of model-scale lengths (>= 2^-60), so is the quotient
  const float cb = gap > 0.f ? div_n(gap, h) : -fminf(div_n(-gap * C.erp, h), C.max_depenetration_velocity);
  const bool warm = gen >= 0 && __float_as_int(wq.w) == 8 * gen + (type == 2 ? CODE_SAMPLE(code) : 0);
  // compact per-contact header for the solve kernel: no dependent model look-ups on its critical path
  if (!FUSED) {
    FLD(clam, 3 * k) = warm ? wq.x : 0.f; FLD(clam, 3 * k + 1) = warm ? wq.y : 0.f; FLD(clam, 3 * k + 2) = warm ? wq.z : 0.f;
    FLD(chdr, 8 * k + 0) = __int_as_float(code | (nFi << 12));
    FLD(chdr, 8 * k + 1) = __int_as_float(f >= 0 ? 4 * f : -1);
    FLD(chdr, 8 * k + 2) = mu_k;
    FLD(chdr, 8 * k + 3) = cb;
  }
  FLD(chdr, 8 * k + 4) = __int_as_float(CODE_FSLOT(code));
  FLD(chdr, 8 * k + 5) = n.x; FLD(chdr, 8 * k + 6) = n.y; FLD(chdr, 8 * k + 7) = n.z;
  if (FUSED) {   // the fused kernel's LDS headers (all KMAX list entries)
    float* s_hdr = sh + FS_HDR * 64;
    float* s_lam = sh + FS_LAM * 64;
    s_hdr[(4 * k) * 64 + lane] = __int_as_float(code | (nFi << 12)); s_hdr[(4 * k + 1) * 64 + lane] = __int_as_float(f >= 0 ? 4 * f : -1);
    s_hdr[(4 * k + 2) * 64 + lane] = mu_k; s_hdr[(4 * k + 3) * 64 + lane] = cb;
    s_lam[(3 * k) * 64 + lane] = warm ? wq.x : 0.f; s_lam[(3 * k + 1) * 64 + lane] = warm ? wq.y : 0.f;
    s_lam[(3 * k + 2) * 64 + lane] = warm ? wq.z : 0.f;
  }
}

__global__ __launch_bounds__(384) void k_dynamics(Arena A, const DevParams* __restrict__ P, int N) {
  __shared__ __attribute__((aligned(16))) float sh[(DL_SPLIT + 1) * 64];   // 16-byte aligned: S^-1 is stored as quads
  constexpr int dlb = DL_PERSIST;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + lane;   // N is the padded stride: every lane owns a (possibly dummy) env
  const DexHandModel& M = P->model;
  const DexSimConfig& C = P->cfg;
  const V3 grav = v3p(C.gravity);
  const bool has_box = C.has_box != 0;
  BaseChain B;
  FingerIn fin;
  if (wv < 5) finger_load(A, wv, N, e, fin);
  base_chain<false>(A, P, grav, N, e, B, wv == 5);

  // ---- phase 1: five finger waves + the palm/box wave, in parallel
  int nc = 0;
  V3 bpos = {0, 0, 0}; M3 Rb = q2mat(Q4{0, 0, 0, 1});
  float hb = 0.f, bmu = 0.f;
  if (wv < 5) {
    finger_dynamics<false>(A, P, B, fin, sh, dlb, nullptr, lane, wv, N, e);
  } else {
    const M3 R5 = q2mat(B.q5);
    Comp comp5;
    comp5.m = P->jc[5].mass;
    comp5.c = B.o5 + mul(R5, v3p(P->jc[5].com));
    comp5.I = rotate_inertia(R5, P->jc[5].inertia);
    V3 rc = comp5.c - B.o5;
    V3 ac = B.ao5 + cross(B.al5, rc) + cross(B.w5, cross(B.w5, rc));
    V3 f5 = comp5.m * ac;
    V3 n5 = mul(comp5.I, B.al5) + cross(B.w5, mul(comp5.I, B.w5)) + cross(rc, f5);
    comp_put(sh, lane, DL_PALM, comp5, B.o5);
    sh_put3(sh, lane, DL_PALM_WRENCH, f5); sh_put3(sh, lane, DL_PALM_WRENCH + 3, n5);
    const float h = P->h;
    if (has_box) {
      bpos = {FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2)};
      Rb = q2mat(Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)});
      hb = 0.5f * C.box_size;
      bmu = FLD(box_mu, 0);
      const float mu_bg = 0.5f * (bmu + C.ground_friction);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        V3 l = {(i & 1) ? hb : -hb, (i & 2) ? hb : -hb, (i & 4) ? hb : -hb};
        V3 p = mul(Rb, l) + bpos;
        if (!C.box_fixed && p.z < C.contact_offset && nc < 4) push_contact(A, N, e, nc, 2, 0, i, p, v3(0, 0, 1), p.z - C.rest_offset, mu_bg, -1, nullptr, DEXSIM_FSLOT_BOX << 21);   // <= 4 box/ground contacts
      }
      const float hg = C.box_fixed ? 0.f : h;   // (static box: no gravity; its velocities are and stay zero)
      FLD(ufree, 26) = FLD(box_lin, 0) + hg * grav.x;
      FLD(ufree, 27) = FLD(box_lin, 1) + hg * grav.y;
      FLD(ufree, 28) = FLD(box_lin, 2) + hg * grav.z;
      FLD(ufree, 29) = FLD(box_ang, 0); FLD(ufree, 30) = FLD(box_ang, 1); FLD(ufree, 31) = FLD(box_ang, 2);
    } else {
#pragma unroll
      for (int i = 26; i < 32; i++) FLD(ufree, i) = 0.f;
    }
  }
  __syncthreads();

  // ---- phase 2: wave 0 reduces + inverts the Schur complement; wave 5 runs the narrowphase meanwhile
  if (wv == 0) schur_base(A, P, B, sh, dlb, nullptr, lane, N, e);
  if (wv == 5) {
    const float mu_hg = 0.5f * (M.hand_friction + C.ground_friction);
    const float mu_hb = 0.5f * (M.hand_friction + bmu);
    const int nbg = nc;
    int cntw[6], tmask = 0;   // hand contacts per finger / palm, which list entries are hand/box contacts
#pragma unroll 1
    for (int f = 0; f < 5; f++) {
      const int n0 = nc;
#pragma unroll 1
      for (int l = 3; l >= 1; l--) {   // distal, middle, proximal
        const int cap = 3 + 3 * f + (l - 1);
        const V3 e0 = sh_get3(sh, lane, DL_CAPS(dlb, f) + 6 * (l - 1)), e1 = sh_get3(sh, lane, DL_CAPS(dlb, f) + 6 * (l - 1) + 3);
        collide_capsule(A, N, e, nc, C, cap, e0, e1, M.cap_r[cap], has_box, bpos, Rb, hb, mu_hb, mu_hg, -1, &tmask, code_info(M, cap));
      }
      if (f == 0) cntw[0] = nc - n0; else if (f == 1) cntw[1] = nc - n0; else if (f == 2) cntw[2] = nc - n0; else if (f == 3) cntw[3] = nc - n0; else cntw[4] = nc - n0;
    }
    const M3 R5 = q2mat(B.q5);
    const int n5 = nc;
#pragma unroll 1
    for (int cpl = 0; cpl < 3; cpl++)
      collide_capsule(A, N, e, nc, C, cpl, B.o5 + mul(R5, v3p(M.cap_p0[cpl])), B.o5 + mul(R5, v3p(M.cap_p1[cpl])), M.cap_r[cpl],
                      has_box, bpos, Rb, hb, mu_hb, mu_hg, -1, &tmask, code_info(M, cpl));
    cntw[5] = nc - n5;
    FLD(ncontact, 0) = nc;
    SH(DL_NC) = __int_as_float(nc);
    const int split = split_pack(nbg, cntw, (int)((unsigned)tmask >> nbg));
    FLD(csplit, 0) = split;
    SH(DL_SPLIT) = __int_as_float(split);
  }
  __syncthreads();

  // ---- phase 3: contact rows, contact k on wave k % 6
  nc = __float_as_int(SH(DL_NC));
  int kmax = nc;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) kmax = max(kmax, __shfl_xor(kmax, s));
  const int split = __float_as_int(SH(DL_SPLIT)), gen = FLD(wgen, 0);
#pragma unroll 1
  for (int k = wv; k < kmax; k += 6) {
    if (k < nc) build_contact_rows<false>(A, P, &B, sh, lane, k, N, e, split, gen);
  }
}

// wave-uniform per-contact masks: does ANY lane couple contact k to the hand / a finger / the box
DI void solve_masks(const float* s_hdr, int nc, int kmax, int lane, unsigned& hand_mask, unsigned& fing_mask, unsigned& box_mask) {
  hand_mask = fing_mask = box_mask = 0;
  for (int k = 0; k < kmax; k++) {
    const int code = __float_as_int(s_hdr[(4 * k) * 64 + lane]), fo = __float_as_int(s_hdr[(4 * k + 1) * 64 + lane]);
    const int type = code & 3;
    const bool act = k < nc;
    if (__any(act && type != 2)) hand_mask |= 1u << k;
    if (__any(act && type != 2 && fo >= 0)) fing_mask |= 1u << k;
    if (__any(act && type != 0)) box_mask |= 1u << k;
  }
}

// The box/ground contacts of a lane (at most 4) held in VGPRs across all sweeps.  The ground is the plane z = 0: every such
// contact has the normal n = +z and therefore the same tangents t1 = (0,-1,0), t2 = (1,0,0) (tangent_basis(+z)); its three rows
// are (d_r, r x d_r) with r = contact point - box centre, so the lever arm r (3 words) is all a contact needs:
//   J_0 v = vz + ry wx - rx wy      J_1 v = -vy + rz wx - rx wz      J_2 v = vx + rz wy - ry wz
// (Round 2 first kept the generic 3 x 6 row words per contact: 72 VGPRs of mostly 0 / +-1 entries; this form needs 12, and
// a sweep ~30 instead of ~55 instructions per contact.)
// load() = the prologue (lever arms, diagonals, in-contact couplings, impulses), sweep() = one Gauss-Seidel pass over them
// against the packed box twist (vx,vy) (vz,wx) (wy,wz), store() = impulses back to LDS.  Used by the early / fast box solves
// and as block 6 of the general contact path (substep_body, phase 4).
struct BoxBlock {
  float rx[4], ry[4], rz[4];
  float Dv[4][3], A10[4], A20[4], A21[4], mu4[4], cb4[4], lam4[4][3];
  float im, iI;   // 1/m, 1/I of the box as this block sees it (split)
  int kms;
  // QUAD: `rows` is the ROWADDR row store with generic rows (k_solve: words ro .. ro+5 of a row = d, r x d), else the compact
  // store [3 k + i][lane] = r_i.
  // nc_lane >= 0: contacts k >= nc_lane of this lane are not initialised in LDS and are taken as absent.
  // resume: start from the impulses in s_lam (warm start / a previous call) instead of from zero.
  // split: the number of solver blocks that share the box in this lane's env (mass splitting: this block sees the box with
  // 1/split of its mass).
  template <bool QUAD>
  DI void load(int kmax, float inv_m, float inv_I, const float* s_lam, const float* s_hdr, const float* rows, int rw, int ro, int lane,
               int nc_lane, bool resume, float split = 1.f) {
    kms = __builtin_amdgcn_readfirstlane(kmax);
    inv_m *= split; inv_I *= split;
    im = inv_m; iI = inv_I;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool use = k < kms && (nc_lane < 0 || k < nc_lane);   // (k < kms: wave-uniform)
      float x = 0.f, y = 0.f, z = 0.f;
      if (k < kms) {
        if (QUAD) {   // r x (0,0,1) = (ry, -rx, 0),  r x (0,-1,0) = (rz, 0, -rx)
          y = rows[ROWADDR((k * 3) * rw + ro + 3, lane)]; x = -rows[ROWADDR((k * 3) * rw + ro + 4, lane)];
          z = rows[ROWADDR((k * 3 + 1) * rw + ro + 3, lane)];
        } else {
          x = rows[(3 * k) * 64 + lane]; y = rows[(3 * k + 1) * 64 + lane]; z = rows[(3 * k + 2) * 64 + lane];
        }
      }
      rx[k] = use ? x : 0.f; ry[k] = use ? y : 0.f; rz[k] = use ? z : 0.f;
      mu4[k] = use ? s_hdr[(4 * k + 2) * 64 + lane] : 0.f;
      cb4[k] = use ? s_hdr[(4 * k + 3) * 64 + lane] : 0.f;
#pragma unroll
      for (int r = 0; r < 3; r++) lam4[k][r] = (use && resume) ? s_lam[(3 * k + r) * 64 + lane] : 0.f;
      const float xx = rx[k] * rx[k], yy = ry[k] * ry[k], zz = rz[k] * rz[k];
      // These three, the row builder's 1/D and tangent_basis stay on the operators although their operands are in rcp_n's range
      // (non-negative terms plus 1e-9): with them on the helpers the register allocator leaves a 36-byte spill slot that no
      // instruction uses in k_physics4<false> or k_physics1<false>, and a launch with any private segment pays for its set-up.
      // None of them is on a finger chain.
      Dv[k][0] = use ? 1.f / (inv_m + inv_I * (xx + yy) + 1e-9f) : 0.f;
      Dv[k][1] = use ? 1.f / (inv_m + inv_I * (xx + zz) + 1e-9f) : 0.f;
      Dv[k][2] = use ? 1.f / (inv_m + inv_I * (yy + zz) + 1e-9f) : 0.f;
      A10[k] = inv_I * ry[k] * rz[k]; A20[k] = -inv_I * rx[k] * rz[k]; A21[k] = inv_I * rx[k] * ry[k];   // A_rs = J_r M^-1 J_s^T
    }
  }
  // one pass over the (up to 4) contacts; the twist is (vx,vy) (vz,wx) (wy,wz)
  // Returns whether the pass changed any impulse of this lane.  A pass is a deterministic map of (impulses, twist); a pass
  // that changes no impulse changes no twist word either (every change of the twist is a multiple of some dl), so once a
  // whole wave reports "no change" every further pass would reproduce the same state: the callers stop there.
  DI bool sweep(f2& v01, f2& v23, f2& v45) {
    float vx = v01.x, vy = v01.y, vz = v23.x, wx = v23.y, wy = v45.x, wz = v45.y;
    bool chg = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k < kms) {   // scalar guard (no break: keeps k a compile-time index, everything stays in VGPRs)
        const float vr0 = vz + ry[k] * wx - rx[k] * wy;
        float vr1 = -vy + rz[k] * wx - rx[k] * wz, vr2 = vx + rz[k] * wy - ry[k] * wz;
        const float nl0 = fmaxf(0.f, lam4[k][0] - (vr0 + cb4[k]) * Dv[k][0]);
        const float dl0 = nl0 - lam4[k][0], lim = mu4[k] * nl0;
        vr1 += A10[k] * dl0; vr2 += A20[k] * dl0;
        const float nl1 = __builtin_amdgcn_fmed3f(lam4[k][1] - vr1 * Dv[k][1], -lim, lim);
        const float dl1 = nl1 - lam4[k][1];
        vr2 += A21[k] * dl1;
        const float nl2 = __builtin_amdgcn_fmed3f(lam4[k][2] - vr2 * Dv[k][2], -lim, lim);
        const float dl2 = nl2 - lam4[k][2];
        lam4[k][0] = nl0; lam4[k][1] = nl1; lam4[k][2] = nl2;
        chg = chg || dl0 != 0.f || dl1 != 0.f || dl2 != 0.f;
        apply(k, dl0, dl1, dl2, f2{im, iI}, vx, vy, vz, wx, wy, wz);
      }
    }
    v01 = f2{vx, vy}; v23 = f2{vz, wx}; v45 = f2{wy, wz};
    return chg;
  }
  // one pass that also accumulates the pass's twist change for the UNSPLIT box (mI0 = its 1/m, 1/I) in d: the block's entry
  // for the exchange, without the cancellation of (v - v_start) / split
  DI void sweep_delta(f2& v01, f2& v23, f2& v45, f2& d01, f2& d23, f2& d45, f2 mI0) {
    float vx = v01.x, vy = v01.y, vz = v23.x, wx = v23.y, wy = v45.x, wz = v45.y;
    float dx = 0.f, dy = 0.f, dz = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k < kms) {
        const float vr0 = vz + ry[k] * wx - rx[k] * wy;
        float vr1 = -vy + rz[k] * wx - rx[k] * wz, vr2 = vx + rz[k] * wy - ry[k] * wz;
        const float nl0 = fmaxf(0.f, lam4[k][0] - (vr0 + cb4[k]) * Dv[k][0]);
        const float dl0 = nl0 - lam4[k][0], lim = mu4[k] * nl0;
        vr1 += A10[k] * dl0; vr2 += A20[k] * dl0;
        const float nl1 = __builtin_amdgcn_fmed3f(lam4[k][1] - vr1 * Dv[k][1], -lim, lim);
        const float dl1 = nl1 - lam4[k][1];
        vr2 += A21[k] * dl1;
        const float nl2 = __builtin_amdgcn_fmed3f(lam4[k][2] - vr2 * Dv[k][2], -lim, lim);
        const float dl2 = nl2 - lam4[k][2];
        lam4[k][0] = nl0; lam4[k][1] = nl1; lam4[k][2] = nl2;
        apply(k, dl0, dl1, dl2, f2{im, iI}, vx, vy, vz, wx, wy, wz);
        apply(k, dl0, dl1, dl2, mI0, dx, dy, dz, ex, ey, ez);
      }
    }
    v01 = f2{vx, vy}; v23 = f2{vz, wx}; v45 = f2{wy, wz};
    d01 = f2{dx, dy}; d23 = f2{dz, ex}; d45 = f2{ey, ez};
  }
  // twist change of the impulse change (dl0, dl1, dl2) of contact k: M^-1 J^T dl
  DI void apply(int k, float dl0, float dl1, float dl2, f2 mI, float& vx, float& vy, float& vz, float& wx, float& wy, float& wz) const {
    const float m0 = mI.x * dl0, m1 = mI.x * dl1, m2 = mI.x * dl2, i0 = mI.y * dl0, i1 = mI.y * dl1, i2 = mI.y * dl2;
    vz += m0; vy -= m1; vx += m2;
    wx += ry[k] * i0 + rz[k] * i1;
    wy += rz[k] * i2 - rx[k] * i0;
    wz -= rx[k] * i1 + ry[k] * i2;
  }
  // warm start: the twist change that goes with the loaded impulses, for the UNSPLIT box (mI = (1/m, 1/I) of the whole box)
  DI void warm(f2& v01, f2& v23, f2& v45, f2 mI) const {
    float vx = v01.x, vy = v01.y, vz = v23.x, wx = v23.y, wy = v45.x, wz = v45.y;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (k < kms) apply(k, lam4[k][0], lam4[k][1], lam4[k][2], mI, vx, vy, vz, wx, wy, wz);
    }
    v01 = f2{vx, vy}; v23 = f2{vz, wx}; v45 = f2{wy, wz};
  }
  // nmine >= 0: only the impulses of this lane's own contacts k < nmine are written (the slots behind them belong to the
  // lane's hand contacts); nmine < 0: all four slots
  DI void store(float* s_lam, int lane, int nmine = -1) const {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (nmine < 0 || k < nmine) {
#pragma unroll
        for (int r = 0; r < 3; r++) s_lam[(3 * k + r) * 64 + lane] = lam4[k][r];
      }
    }
  }
};

// warm-start cache of the lane's nmine box/ground contacts, from the impulses in s_lam: slot 80 + k <- (impulses, 8 * gen +
// corner of slot k (cpack))
DI void cache_box_ground(const Arena& A, const float* s_lam, int gen, int cpack, int nmine, int lane, int N, int e) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k < nmine)
      st4_global(A.wlam + ((size_t)(80 + k) * N + e) * 4, s_lam[(3 * k) * 64 + lane], s_lam[(3 * k + 1) * 64 + lane], s_lam[(3 * k + 2) * 64 + lane],
                 __int_as_float(8 * gen + ((cpack >> (3 * k)) & 7)));
  }
}

// net contact force per body of the last sub-step (contact_collection: CC_LAST_SUBSTEP); the slot index is data
// dependent per lane -> accumulate in LDS scratch s_f [51][64]
DI void solve_forces(const Arena& A, const DevParams* __restrict__ P, int* __restrict__ cnt, const float* s_hdr, const float* s_lam,
                     float* s_f, int nc, int lane, int N, int e, int NR) {
  const float h = P->h;
#pragma unroll
  for (int i = 0; i < DEXSIM_NFSLOT * 3; i++) s_f[i * 64 + lane] = 0.f;
  int nhand = 0;
  for (int k = 0; k < nc; k++) {
    const int type = __float_as_int(s_hdr[(4 * k) * 64 + lane]) & 3;
    nhand += type < 2 ? 1 : 0;
    if (type == 3) continue;   // a joint-limit reaction is a joint torque, not a force on a body
    const int slot = __float_as_int(FLD(chdr, 8 * k + 4));
    const V3 n = {FLD(chdr, 8 * k + 5), FLD(chdr, 8 * k + 6), FLD(chdr, 8 * k + 7)};
    V3 t1, t2;
    tangent_basis(n, t1, t2);
    const float l0 = s_lam[(3 * k) * 64 + lane] / h, l1 = s_lam[(3 * k + 1) * 64 + lane] / h, l2 = s_lam[(3 * k + 2) * 64 + lane] / h;
    const V3 F = l0 * n + l1 * t1 + l2 * t2;
    s_f[(3 * slot) * 64 + lane] += F.x; s_f[(3 * slot + 1) * 64 + lane] += F.y; s_f[(3 * slot + 2) * 64 + lane] += F.z;
    if (type == 1) {
      s_f[(3 * DEXSIM_FSLOT_BOX) * 64 + lane] -= F.x; s_f[(3 * DEXSIM_FSLOT_BOX + 1) * 64 + lane] -= F.y;
      s_f[(3 * DEXSIM_FSLOT_BOX + 2) * 64 + lane] -= F.z;
    }
  }
#pragma unroll
  for (int i = 0; i < DEXSIM_NFSLOT * 3; i++) FLD(cforce, i) = s_f[i * 64 + lane];
  if (cnt) {   // cnt = counters + stamp parity (null in gated launches); padded lanes (e >= NR) are not counted
    int tot = e < NR ? (nc | (nhand << 16)) : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) tot += __shfl_xor(tot, s);
    if (lane == 0) { atomicAdd(&cnt[CNT_CONTACTS], tot & 0xffff); if (tot >> 16) atomicAdd(&cnt[CNT_HAND_CONTACTS], tot >> 16); }
  }
}

// solve_forces for the early box solve: every contact is box/ground (slot = box, normal = +z), so the only non-zero
// row group is the box's; same accumulation order as solve_forces.  Runs on the box wave right behind its sweeps.
DI void solve_forces_box(const Arena& A, const DevParams* __restrict__ P, int* __restrict__ cnt, const float* s_lam, int nc, int lane, int N,
                         int e, int NR) {
  const float h = P->h;
  V3 n = v3(0, 0, 1), t1, t2;
  tangent_basis(n, t1, t2);
  V3 acc = {0.f, 0.f, 0.f};
  for (int k = 0; k < nc; k++) {
    const float l0 = s_lam[(3 * k) * 64 + lane] / h, l1 = s_lam[(3 * k + 1) * 64 + lane] / h, l2 = s_lam[(3 * k + 2) * 64 + lane] / h;
    const V3 F = l0 * n + l1 * t1 + l2 * t2;
    acc.x += F.x; acc.y += F.y; acc.z += F.z;
  }
#pragma unroll
  for (int i = 0; i < DEXSIM_NFSLOT * 3; i++) FLD(cforce, i) = 0.f;
  FLD(cforce, 3 * DEXSIM_FSLOT_BOX) = acc.x; FLD(cforce, 3 * DEXSIM_FSLOT_BOX + 1) = acc.y; FLD(cforce, 3 * DEXSIM_FSLOT_BOX + 2) = acc.z;
  if (cnt) {
    int tot = e < NR ? nc : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) tot += __shfl_xor(tot, s);
    if (lane == 0) atomicAdd(&cnt[CNT_CONTACTS], tot);
  }
}

// solve_forces of the fused general path, spread over waves 0-4: wave w adds up the forces of list entries w, w + 5, ... in a
// scratch block of its own (s_f + w * 51 rows); all of a wave's header loads (force slot, normal: arena) are in flight at once.
// forces_reduce (one wave, after a barrier) adds the five blocks in wave order and writes the result: fixed order, bit-reproducible.
DI void forces_partial(const Arena& A, const DevParams* __restrict__ P, const float* s_hdr, const float* s_lam, float* s_f, int nc, int w,
                       int lane, int N, int e) {
  const float rh = rcp_n(P->h);   // the sub-step, 1e-4 .. 1e-1 s
#pragma unroll
  for (int i = 0; i < DEXSIM_NFSLOT * 3; i++) s_f[i * 64 + lane] = 0.f;
  int slot[5];
  V3 nn[5];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int k = w + 5 * i;
    const bool act = k < nc;
    slot[i] = act ? __float_as_int(FLD(chdr, 8 * k + 4)) : 0;
    nn[i] = act ? V3{FLD(chdr, 8 * k + 5), FLD(chdr, 8 * k + 6), FLD(chdr, 8 * k + 7)} : V3{0.f, 0.f, 1.f};
  }
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const int k = w + 5 * i;
    if (k < nc) {
      const int type = __float_as_int(s_hdr[(4 * k) * 64 + lane]) & 3;
      if (type == 3) continue;   // a joint-limit reaction is a joint torque, not a force on a body
      V3 t1, t2;
      tangent_basis(nn[i], t1, t2);
      const float l0 = s_lam[(3 * k) * 64 + lane] * rh, l1 = s_lam[(3 * k + 1) * 64 + lane] * rh, l2 = s_lam[(3 * k + 2) * 64 + lane] * rh;
      const V3 F = l0 * nn[i] + l1 * t1 + l2 * t2;
      const int sl = slot[i];
      s_f[(3 * sl) * 64 + lane] += F.x; s_f[(3 * sl + 1) * 64 + lane] += F.y; s_f[(3 * sl + 2) * 64 + lane] += F.z;
      if (type == 1) {
        s_f[(3 * DEXSIM_FSLOT_BOX) * 64 + lane] -= F.x; s_f[(3 * DEXSIM_FSLOT_BOX + 1) * 64 + lane] -= F.y;
        s_f[(3 * DEXSIM_FSLOT_BOX + 2) * 64 + lane] -= F.z;
      }
    }
  }
}
// w0 / nw: this wave's share of the 51 force words -- w0, w0 + nw, ... (the five finger waves take a fifth each: on wave 0 alone the
// sums were a 7.7k-cycle tail of the last sub-step of every general-path physics step, behind which the publication waited)
DI void forces_reduce(const Arena& A, int* __restrict__ cnt, const float* s_hdr, const float* s_f, int nc, int lane, int N, int e, int NR,
                      int w0 = 0, int nw = 1) {
#pragma unroll 3
  for (int i = w0; i < DEXSIM_NFSLOT * 3; i += nw) {
    float v = s_f[i * 64 + lane];
#pragma unroll
    for (int w = 1; w < 5; w++) v += s_f[(w * DEXSIM_NFSLOT * 3 + i) * 64 + lane];
    FLD(cforce, i) = v;
  }
}
// contact statistics of the general path (one wave; in the fused kernel the palm wave, whose phase 5 is the shortest)
DI void contact_stats(int* __restrict__ cnt, const float* s_hdr, int nc, int lane, int e, int NR) {
  if (cnt) {   // cnt = counters + stamp parity (null in gated launches); padded lanes (e >= NR) are not counted
    int nhand = 0;
    for (int k = 0; k < nc; k++) nhand += (__float_as_int(s_hdr[(4 * k) * 64 + lane]) & 3) < 2 ? 1 : 0;   // (joint-limit rows are not contacts)
    int tot = e < NR ? (nc | (nhand << 16)) : 0;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) tot += __shfl_xor(tot, s);
    if (lane == 0) { atomicAdd(&cnt[CNT_CONTACTS], tot & 0xffff); if (tot >> 16) atomicAdd(&cnt[CNT_HAND_CONTACTS], tot >> 16); }
  }
}

// (q_new / qd_new, if given: the integrated state, for the next inlined sub-step body -- see SubstepCarry)
// store = false (bodies 1-3 of a fused launch): the new state goes on to the next body in registers / LDS only (SubstepCarry); nothing
// reads the arena's q, qd before the last body has written them
DI void integrate_joint(const Arena& A, const DevParams* __restrict__ P, float h, int j, float q0, float v, int N, int e,
                        float* q_new = nullptr, float* qd_new = nullptr, bool store = true) {
  float qn = q0 + h * v;
  const float lo = P->jc[j].lo, hi = P->jc[j].hi;
  if (qn < lo) { qn = lo; v = fmaxf(v, 0.f); }
  if (qn > hi) { qn = hi; v = fminf(v, 0.f); }
  if (store) { FLD(q, j) = qn; FLD(qd, j) = v; }
  if (q_new) { *q_new = qn; *qd_new = v; }
}
DI void integrate_box(const Arena& A, float h, const float* vb, const float* wb, int N, int e) {
#pragma unroll
  for (int i = 0; i < 3; i++) { FLD(box_lin, i) = vb[i]; FLD(box_ang, i) = wb[i]; FLD(box_pos, i) = fmaf(h, vb[i], FLD(box_pos, i)); }   // (explicit fma: the fused kernel's carried copy below must be the same bits)
  Q4 bq = {FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)};
  Q4 dq = qmul(Q4{wb[0], wb[1], wb[2], 0.f}, bq);
  Q4 qn = {bq.x + 0.5f * h * dq.x, bq.y + 0.5f * h * dq.y, bq.z + 0.5f * h * dq.z, bq.w + 0.5f * h * dq.w};
  // a unit quaternion plus an increment orthogonal to it: l >= 1 - rounding, every |component| <= l (zero components stay zero)
  float l = sqrt_n(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);
  FLD(box_quat, 0) = div_n(qn.x, l); FLD(box_quat, 1) = div_n(qn.y, l); FLD(box_quat, 2) = div_n(qn.z, l); FLD(box_quat, 3) = div_n(qn.w, l);
}

// Stand-alone contact-solve kernel (profiling / staged tests; production runs the fused k_physics4 / k_physics1 below):
// reads u_free, headers and rows from the arena, stages them in LDS, sweeps, integrates.
__global__ __launch_bounds__(64) void k_solve(Arena A, const DevParams* __restrict__ P, int* __restrict__ cnt, int stamp, int kstage,
                                              int N, int NR) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int e = blockIdx.x * 64 + lane;
  float* s_uf = lds;                         // [20][64]  finger velocities in u-space (+ [20] block copy, [20] block changes)
  float* s_lam = lds + 60 * 64;              // [KMAX*3][64]  impulses
  float* s_hdr = lds + (60 + DEXSIM_KMAX * 3) * 64;   // [KMAX*4][64]  per contact: code, finger offset, mu, bias
  float* s_row = lds + (60 + DEXSIM_KMAX * 3 + DEXSIM_KMAX * 4) * 64;   // [kstage*84][64] staged row data
  const DexSimConfig& C = P->cfg;
  const float h = P->h;
  const bool has_box = C.has_box != 0;

  float uB[6], vb[3], wb[3];
#pragma unroll
  for (int i = 0; i < 6; i++) uB[i] = FLD(ufree, i);
#pragma unroll
  for (int i = 0; i < 20; i++) s_uf[i * 64 + lane] = FLD(ufree, 6 + i);
#pragma unroll
  for (int i = 0; i < 3; i++) { vb[i] = FLD(ufree, 26 + i); wb[i] = FLD(ufree, 29 + i); }
  const int nc = FLD(ncontact, 0);
  float inv_m = 0.f, inv_I = 0.f;
  if (has_box && !C.box_fixed) { inv_m = rcp_n(FLD(box_mass, 0)); inv_I = P->box_inv_I_k * inv_m; }   // a body mass in kg
  int kmax = nc;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) kmax = max(kmax, __shfl_xor(kmax, s));
  const int kst = min(kmax, kstage);
  for (int k = 0; k < kmax * 3; k++) s_lam[k * 64 + lane] = k < nc * 3 ? FLD(clam, k) : 0.f;   // starting impulses (warm start, k_dynamics)
  // contact headers (inactive slots: type 2 with zero everything): one batch of independent coalesced loads
#pragma unroll 4
  for (int k = 0; k < kmax; k++) {
    const bool act = k < nc;
    const float w0 = act ? FLD(chdr, 8 * k + 0) : __int_as_float(2), w1 = act ? FLD(chdr, 8 * k + 1) : __int_as_float(0);
    const float w2 = act ? FLD(chdr, 8 * k + 2) : 0.f, w3 = act ? FLD(chdr, 8 * k + 3) : 0.f;
    s_hdr[(4 * k) * 64 + lane] = w0; s_hdr[(4 * k + 1) * 64 + lane] = w1;
    s_hdr[(4 * k + 2) * 64 + lane] = w2; s_hdr[(4 * k + 3) * 64 + lane] = w3;
  }
  unsigned hand_mask, fing_mask, box_mask;
  solve_masks(s_hdr, nc, kmax, lane, hand_mask, fing_mask, box_mask);
  // stage rows: coalesced 256-B transactions, a whole contact's words in flight at once (v1 of this loop kept
  // only 8 loads in flight and was L2-latency bound).  Contacts that no lane of the wavefront couples to the
  // hand (e.g. the 4 box/ground contacts of a resting box) only need their 7 box words per row.
  for (int k = 0; k < kst; k++) {
    const int base = k * 3 * CROW_W;
    const bool act = k < nc;   // lanes without this contact stage zeros (=> zero impulse, branch-free sweeps)
    if ((hand_mask >> k) & 1) {
      float tmp[3 * CROW_W];
#pragma unroll
      for (int w = 0; w < 3 * CROW_W; w++) tmp[w] = act ? FLD(crow, base + w) : 0.f;
#pragma unroll
      for (int w = 0; w < 3 * CROW_W; w++) s_row[ROWADDR(base + w, lane)] = tmp[w];
    } else {
      float tmp[24];   // 7 box words + the in-contact coupling (pad word 27) per row
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int w = 0; w < 8; w++) tmp[8 * r + w] = act ? FLD(crow, base + r * CROW_W + 20 + w) : 0.f;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int w = 0; w < 8; w++) s_row[ROWADDR(base + r * CROW_W + 20 + w, lane)] = tmp[8 * r + w];
    }
  }
  const int gen = FLD(wgen, 0);
  int nbg = 0;      // box/ground contacts lead the list
  for (int k = 0; k < min(kmax, 4); k++) nbg += (k < nc && (__float_as_int(s_hdr[(4 * k) * 64 + lane]) & 3) == 2) ? 1 : 0;
  if (hand_mask == 0 && kmax <= 4 && kmax <= kst) {
    // ---- only box/ground contacts in the whole wavefront: one block, nothing is split (the early box solve of the fused kernel)
    // (nc_lane = nc: a lane with fewer contacts than the wave's kmax has zero rows staged for the slots behind its own, but the block
    // computes 1/D itself -- 1 / (1/m + 1e-9) for a zero lever arm -- so a slot taken as present would act as a frictionless support
    // under the box centre whenever the box moves down)
    BoxBlock bb;
    bb.load<true>(kmax, inv_m, inv_I, s_lam, s_hdr, s_row, CROW_W, 20, lane, nc, true);
    f2 v01 = {vb[0], vb[1]}, v23 = {vb[2], wb[0]}, v45 = {wb[1], wb[2]};
    bb.warm(v01, v23, v45, f2{inv_m, inv_I});
#pragma unroll 1
    for (int it = 0; it < C.num_position_iterations; it++) bb.sweep(v01, v23, v45);
    vb[0] = v01.x; vb[1] = v01.y; vb[2] = v23.x; wb[0] = v23.y; wb[1] = v45.x; wb[2] = v45.y;
    bb.store(s_lam, lane);
  } else {
    // ---- the block solver of the fused kernel's phase 4, block after block on this one wave (rows streamed from the arena
    // by per-lane list entry; a test / profiling kernel: clarity over speed)
    const int split = FLD(csplit, 0), rs = SPLIT_RS(split), nh = nc - nbg;
    const float nBf = (float)SPLIT_NB(split), nXf = (float)SPLIT_NX(split);
    float* s_ufl = s_uf + 20 * 64;   // the current block's copy of the finger velocities
    float* s_ufd = s_uf + 40 * 64;   // sum of the blocks' changes to them
    // one contact (list entry k of this lane, act = it exists) against the velocities (U, Vb, Wb, finger words in `uf`), with the
    // response scaled by (sB, sF, sX); mode 0 = add the effect of the current impulses (warm start), 1 = projected update
    auto contact = [&](int k, bool act, float (&U)[6], float (&Vb)[3], float (&Wb)[3], float* uf, float sB, float sX, int mode) {
      const int kk = act ? k : 0;
      const int code = __float_as_int(s_hdr[(4 * kk) * 64 + lane]), fo = __float_as_int(s_hdr[(4 * kk + 1) * 64 + lane]);
      const float mu = s_hdr[(4 * kk + 2) * 64 + lane], cb = s_hdr[(4 * kk + 3) * 64 + lane];
      const float sF = mode ? (float)((code >> 12) & 15) : 1.f;
      const bool fing = act && fo >= 0;
      const int foe = max(fo, 0);
      float lam_n = 0.f;
      for (int r = 0; r < 3; r++) {
        const float* rp = A.crow + (size_t)((kk * 3 + r) * CROW_W) * N + e;
        float row[CROW_W];
        for (int w = 0; w < CROW_W; w++) row[w] = act ? rp[(size_t)w * N] : 0.f;
        float lam = act ? s_lam[(3 * kk + r) * 64 + lane] : 0.f, dl;
        if (mode) {
          float vr = 0.f;
          for (int i = 0; i < 6; i++) vr += row[i] * U[i];
          for (int l = 0; l < 4; l++) vr += row[6 + l] * uf[(foe + l) * 64 + lane];
          for (int i = 0; i < 3; i++) vr += row[20 + i] * Vb[i] + row[23 + i] * Wb[i];
          float nl;
          if (r == 0) { nl = fmaxf(0.f, lam - (vr + cb) * row[26]); lam_n = nl; }
          else { const float lim = mu * lam_n; nl = clampf(lam - vr * row[26], -lim, lim); }
          dl = nl - lam;
          if (act) s_lam[(3 * kk + r) * 64 + lane] = nl;
        } else dl = lam;
        for (int i = 0; i < 6; i++) U[i] += row[10 + i] * (sB * dl);
        if (fing) for (int l = 0; l < 4; l++) uf[(foe + l) * 64 + lane] += row[16 + l] * (sF * dl);
        for (int i = 0; i < 3; i++) { Vb[i] += row[20 + i] * (sX * inv_m * dl); Wb[i] += row[23 + i] * (sX * inv_I * dl); }
      }
    };
    // warm start: plain sum over all contacts, unsplit
    for (int k = 0; k < kmax; k++) contact(k, k < nc, uB, vb, wb, s_uf, 1.f, 1.f, 0);
    for (int i = 0; i < 20; i++) s_ufd[i * 64 + lane] = 0.f;
#pragma unroll 1
    for (int it = 0; it < C.num_position_iterations; it++) {
      float dU[6] = {0, 0, 0, 0, 0, 0}, dV[3] = {0, 0, 0}, dW[3] = {0, 0, 0};
#pragma unroll 1
      for (int b = 0; b < 13; b++) {   // hand blocks 0-11, box/ground block 12
        if (b < 12 && !__any((b << rs) < nh)) continue;
        float U[6], Vb[3], Wb[3];
        for (int i = 0; i < 6; i++) U[i] = uB[i];
        for (int i = 0; i < 3; i++) { Vb[i] = vb[i]; Wb[i] = wb[i]; }
        for (int i = 0; i < 20; i++) s_ufl[i * 64 + lane] = s_uf[i * 64 + lane];
        for (int i = 0; i < 4; i++) {
          const int k = b == 12 ? i : nbg + (b << rs) + i;
          const bool act = b == 12 ? i < nbg : (i < (1 << rs) && (b << rs) + i < nh);
          if (__any(act)) contact(k, act, U, Vb, Wb, s_ufl, nBf, nXf, 1);
        }
        for (int i = 0; i < 6; i++) dU[i] += (U[i] - uB[i]) / nBf;
        for (int i = 0; i < 3; i++) { dV[i] += (Vb[i] - vb[i]) / nXf; dW[i] += (Wb[i] - wb[i]) / nXf; }
        for (int i = 0; i < 20; i++) s_ufd[i * 64 + lane] += (s_ufl[i * 64 + lane] - s_uf[i * 64 + lane]) / (float)SPLIT_NF(split, i >> 2);
      }
      for (int i = 0; i < 6; i++) uB[i] += dU[i];
      for (int i = 0; i < 3; i++) { vb[i] += dV[i]; wb[i] += dW[i]; }
      for (int i = 0; i < 20; i++) { s_uf[i * 64 + lane] += s_ufd[i * 64 + lane]; s_ufd[i * 64 + lane] = 0.f; }
    }
    // warm-start cache of the hand contacts
    for (int k = nbg; k < kmax; k++) {
      if (k < nc) {
        const int code = __float_as_int(s_hdr[(4 * k) * 64 + lane]);
        st4_global(A.wlam + ((size_t)CODE_HKEY(code) * N + e) * 4, s_lam[(3 * k) * 64 + lane], s_lam[(3 * k + 1) * 64 + lane], s_lam[(3 * k + 2) * 64 + lane],
                   __int_as_float(8 * DEXSIM_WGEN_NEXT(gen)));
      }
    }
  }
  {   // warm-start cache of the box/ground contacts (slot = list index, corner in the tag); the generation advances
    int cpack = 0;
    for (int k = 0; k < 4; k++) if (k < nbg) cpack |= CODE_SAMPLE(__float_as_int(s_hdr[(4 * k) * 64 + lane])) << (3 * k);
    cache_box_ground(A, s_lam, DEXSIM_WGEN_NEXT(gen), cpack, nbg, lane, N, e);
    FLD(wgen, 0) = DEXSIM_WGEN_NEXT(gen);
  }

  solve_forces(A, P, cnt + (stamp & 1), s_hdr, s_lam, s_row /* dead by now */, nc, lane, N, e, NR);

  // back-substitution qd = L^-1 u, semi-implicit Euler, joint-limit clamp
#pragma unroll
  for (int i = 0; i < 6; i++) integrate_joint(A, P, h, i, FLD(q, i), uB[i], N, e);
#pragma unroll
  for (int f = 0; f < 5; f++) {
#pragma unroll
    for (int l = 0; l < 4; l++) {
      float v = s_uf[(4 * f + l) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 6; i++) v -= GPTR(A.fac_g)[((size_t)(6 * f + ((l * 6 + i) >> 2)) * N + e) * 4 + ((l * 6 + i) & 3)] * uB[i];   // (quad layout: FQ)
      integrate_joint(A, P, h, 6 + 4 * f + l, FLD(q, 6 + 4 * f + l), v, N, e);
    }
  }
  if (has_box && !C.box_fixed) integrate_box(A, h, vb, wb, N, e);
}

// ------------------------------------------------------------------------------------------------- publish
DI void store_pose(const Arena& A, int N, int e, int s, V3 p, Q4 q) {
  FLD(site_pose, 7 * s + 0) = p.x; FLD(site_pose, 7 * s + 1) = p.y; FLD(site_pose, 7 * s + 2) = p.z;
  FLD(site_pose, 7 * s + 3) = q.x; FLD(site_pose, 7 * s + 4) = q.y; FLD(site_pose, 7 * s + 5) = q.z;
  FLD(site_pose, 7 * s + 6) = q.w;
}

// full_bodies != 0 additionally materialises rigid_body_states (N,B,13) and contact_forces_all (N,B,3)
// 6 wavefronts per 64 envs like k_dynamics: wave f < 5 walks finger f, wave 5 publishes the base chain, the hand
// base site/twist and the actor roots.  Every wave recomputes the 6-joint base chain.
// root_wave: who writes the actor root states -- wave 5 in the 6-wave k_publish; the box wave (6) in the 7-wave fused kernels, where
// wave 5's share (base joints, hand site, hand twist AND the 26 scattered root words) made it the last to reach the barrier in front
// of the post block by ~2k cycles while the box wave had nothing to publish
DI void publish_body(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int full_bodies_req, int N, int NR, int root_wave = 5) {
  const int wv = __builtin_amdgcn_readfirstlane(wave_role(threadIdx.x >> 6));
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const bool w5 = wv == 5;
  const bool real = e < NR;   // padded lanes keep their arena fields valid but never touch the API tensors
  const int full_bodies = full_bodies_req && real;
  const DexHandModel& M = P->model;
  const DexSimConfig& C = P->cfg;
  const int NB = DEXSIM_NUM_HAND_BODIES + (C.has_box ? 1 : 0);
  float* rbs = full_bodies ? T.rigid_body_states + (size_t)e * NB * 13 : nullptr;
  float* cfa = full_bodies ? T.contact_forces_all + (size_t)e * NB * 3 : nullptr;
  auto put_roots = [&]() {   // actor root states: hand actor root = the fixed spawn frame; box = free body
    const int NA = 1 + (C.has_box ? 1 : 0);
    float* root = T.root_state + (size_t)e * NA * 13;
    root[0] = M.spawn_pos[0]; root[1] = M.spawn_pos[1]; root[2] = M.spawn_pos[2];
    root[3] = M.spawn_quat[0]; root[4] = M.spawn_quat[1]; root[5] = M.spawn_quat[2]; root[6] = M.spawn_quat[3];
#pragma unroll
    for (int i = 7; i < 13; i++) root[i] = 0.f;
    if (C.has_box) {
      float* b = root + 13;
      float bs[13];
#pragma unroll
      for (int i = 0; i < 3; i++) { bs[i] = FLD(box_pos, i); bs[7 + i] = FLD(box_lin, i); bs[10 + i] = FLD(box_ang, i); }
#pragma unroll
      for (int i = 0; i < 4; i++) bs[3 + i] = FLD(box_quat, i);
#pragma unroll
      for (int i = 0; i < 13; i++) b[i] = bs[i];
      if (full_bodies) {
        float* d = rbs + DEXSIM_NUM_HAND_BODIES * 13;
#pragma unroll
        for (int i = 0; i < 13; i++) d[i] = bs[i];
        float* c = cfa + DEXSIM_NUM_HAND_BODIES * 3;
#pragma unroll
        for (int i = 0; i < 3; i++) c[i] = FLD(cforce, 3 * DEXSIM_FSLOT_BOX + i);
      }
    }
  };
  if (wv > 5) {   // the fused kernels' 7th wave (the box solver)
    if (wv == root_wave && real) put_roots();
    return;
  }

  auto put_body = [&](int b, V3 o, Q4 q, V3 vo, V3 w) { // body welded to a joint frame (o, q) with twist (vo @ o, w)
    const M3 R = q2mat(q);
    const V3 p = o + mul(R, v3p(M.body_p[b]));
    const Q4 bq = qmul(q, q4p(M.body_q[b]));
    const V3 v = vo + cross(w, p - o);
    float* d = rbs + b * 13;
    d[0] = p.x; d[1] = p.y; d[2] = p.z; d[3] = bq.x; d[4] = bq.y; d[5] = bq.z; d[6] = bq.w;
    d[7] = v.x; d[8] = v.y; d[9] = v.z; d[10] = w.x; d[11] = w.y; d[12] = w.z;
    const int s = M.body_fslot[b];
    float* c = cfa + b * 3;
    c[0] = s >= 0 ? FLD(cforce, 3 * s) : 0.f; c[1] = s >= 0 ? FLD(cforce, 3 * s + 1) : 0.f; c[2] = s >= 0 ? FLD(cforce, 3 * s + 2) : 0.f;
  };

  Q4 qc = q4p(M.spawn_quat);
  V3 oc = v3p(M.spawn_pos);
  V3 w = {0, 0, 0}, vo = {0, 0, 0}; // twist of the current frame: linear velocity of its origin, angular velocity
  if (full_bodies && w5) put_body(0, oc, qc, vo, w);
  int j_first = 0;
  if (!full_bodies_req) {   // step path: joints 0-3 in closed form (see base_chain); the per-body frames are not needed
    float qb[4], qdb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { qb[j] = FLD(q, j); qdb[j] = FLD(qd, j); }
    V3 t = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 3; j++) { t += qb[j] * v3p(P->base_A[j]); vo += qdb[j] * v3p(P->base_A[j]); }
    oc = v3p(P->base_Oc[3]) + t;
    const V3 ax = v3p(P->jc[3].axis);
    float s, c;
    sincos_joint(0.5f * qb[3], &s, &c);
    qc = qmul(q4p(P->base_Q3z), Q4{ax.x * s, ax.y * s, ax.z * s, c});
    w = qdb[3] * v3p(P->base_A[3]);
    if (real && w5) {
#pragma unroll
      for (int j = 0; j < 4; j++) { T.dof_state[((size_t)e * 26 + j) * 2] = qb[j]; T.dof_state[((size_t)e * 26 + j) * 2 + 1] = qdb[j]; }
    }
    j_first = 4;
  }
#pragma unroll
  for (int j = 0; j < 6; j++) {
    if (j < j_first) continue;
    const float qj = FLD(q, j), qdj = FLD(qd, j);
    M3 Rp = q2mat(qc);
    V3 on = oc + mul(Rp, v3p(P->jc[j].poff));
    Q4 qz = qmul(qc, q4p(P->jc[j].qoff));
    V3 ax = v3p(P->jc[j].axis);
    V3 aw = mul(q2mat(qz), ax);
    Q4 qn = qz;
    if (j < 3) on += qj * aw;
    else { float s, c; sincos_joint(0.5f * qj, &s, &c); qn = qmul(qz, Q4{ax.x * s, ax.y * s, ax.z * s, c}); }
    vo = vo + cross(w, on - oc);
    if (j < 3) vo += qdj * aw; else w += qdj * aw;
    qc = qn; oc = on;
    if (full_bodies && w5) put_body(j < 5 ? j + 1 : 6, oc, qc, vo, w);
    if (real && w5) { T.dof_state[((size_t)e * 26 + j) * 2] = qj; T.dof_state[((size_t)e * 26 + j) * 2 + 1] = qdj; }
  }
  const Q4 q5 = qc; const V3 o5 = oc, wb5 = w, v5 = vo;
  if (w5) {
    store_pose(A, N, e, 0, o5 + mul(q2mat(q5), v3p(M.site_p[0])), qmul(q5, q4p(M.site_q[0])));
    const V3 ps = o5 + mul(q2mat(q5), v3p(M.site_p[0]));
    const V3 v = v5 + cross(wb5, ps - o5);
    FLD(hand_vel, 0) = v.x; FLD(hand_vel, 1) = v.y; FLD(hand_vel, 2) = v.z;
    FLD(hand_vel, 3) = wb5.x; FLD(hand_vel, 4) = wb5.y; FLD(hand_vel, 5) = wb5.z;
  } else {
    const int f = wv;
    Q4 qf = q5; V3 of = o5, wf = wb5, vf = v5;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int j = 6 + 4 * f + l;
      const float qj = FLD(q, j), qdj = FLD(qd, j);
      M3 Rp = q2mat(qf);
      V3 on = of + mul(Rp, v3p(P->jc[j].poff));
      Q4 qz = qmul(qf, q4p(P->jc[j].qoff));
      V3 ax = v3p(P->jc[j].axis);
      V3 aw = mul(q2mat(qz), ax);
      float s, c;
      sincos_joint(0.5f * qj, &s, &c);
      Q4 qn = qmul(qz, Q4{ax.x * s, ax.y * s, ax.z * s, c});
      vf = vf + cross(wf, on - of);
      wf += qdj * aw;
      qf = qn; of = on;
      if (full_bodies) put_body(7 + 6 * f + l, of, qf, vf, wf);
      if (real) { T.dof_state[((size_t)e * 26 + j) * 2] = qj; T.dof_state[((size_t)e * 26 + j) * 2 + 1] = qdj; }
    }
    const M3 R = q2mat(qf);
    store_pose(A, N, e, 1 + f, of + mul(R, v3p(M.site_p[1 + f])), qmul(qf, q4p(M.site_q[1 + f])));
    store_pose(A, N, e, 6 + f, of + mul(R, v3p(M.site_p[6 + f])), qmul(qf, q4p(M.site_q[6 + f])));
    if (full_bodies) { put_body(7 + 6 * f + 4, of, qf, vf, wf); put_body(7 + 6 * f + 5, of, qf, vf, wf); }
  }
  if (real && w5 && root_wave == 5) put_roots();
}

__global__ __launch_bounds__(384) void k_publish(Arena A, ApiPtrs T, const DevParams* __restrict__ P, const int* __restrict__ cnt,
                                                 int full_bodies_req, int N, int NR) {
  publish_body(A, T, P, full_bodies_req, N, NR);
}


// ------------------------------------------------------------------------------------------------- fused sub-step
// Production path: dynamics + contact solve + integration of one sub-step in ONE launch, seven waves per 64 envs (roles: finger
// 0-4, palm + base joints, box -- wave_role).
//   phase 0  waves 0-5: base chain, hand-level broadphase | box wave: box state, box/ground contacts (lever arms), warm-start cache
//   phase 1  finger waves: finger dynamics + capsule-level broadphase verdict | palm wave: palm composite | box wave: speculative
//            box/ground solve
//   phase 2  wave 0: Schur complement, u_B | hand clear: box wave finishes its solve (phases 3-4 vanish)
//            | else: narrowphase (a wave's own three capsules; finger 0's on the box wave), ordered append, split counts, work items
//   phase 3  (general path) rows of the hand contacts, one work item = one solver block, dealt densely over the lanes of waves 0-5
//   phase 4  (general path) 1 + 16 passes of the block solver: items update their block, exchange (barrier, reduction, barrier)
//   phase 5  finger waves: back-substitute + integrate finger f | palm wave: base DOFs | box wave: box | (last sub-step) contact forces
// Compared with k_dynamics + k_solve this removes one launch per sub-step and the HBM/L2 round trip of the free velocity and the
// factors between the two kernels.
// LDS words: the LDS map (above finger_dynamics).  XQ(b, q): quad q of block b of the exchange; TQ(q): quad q of the common
// velocities.
#define XQ(b, q) ((f4*)(sh + FS_X * 64 + (((b) * 5 + (q)) * 64 + lane) * 4))
#define TQ(q) ((f4*)(sh + FS_T * 64 + ((q) * 64 + lane) * 4))

// LAST = the final sub-step of a sim.dt: it also accumulates the net contact forces (CC_LAST_SUBSTEP) and ends with
// the site / dof_state / root publication (k_publish's body), so a physics step is `substeps` launches and nothing
// else.  (Running all sub-steps in a runtime loop inside one launch was measured and rejected: keeping the kernel
// arguments and loop invariants live across iterations cost 0.7-2 kB/lane of scratch spills, 45 -> 61 us per
// sub-step; a launch boundary costs ~2 us.)
DI void post_pre_tasks(const Arena& A, const DevParams* __restrict__ P, const int* __restrict__ cnt, float* s_ob, int N);   // dexsim_l2.hip.inc
#define POST_PRE_MASK 0x01   /* post task 0 (it reads nothing the publication writes, dexsim_l2.hip.inc): run by the box wave next to
                                the publication.  (Round 2/3 also ran tasks 2, 3, 4, 5 there: the box wave then reached the barrier in front of
                                the post block 4.6k cycles after the finger waves, while helper wave 1 of the post block's phase A -- whose
                                tasks these are -- sat idle for the 10k cycles of wave 0's loads and logic.) */

// ---- block-parallel sweeps of the fused general path (substep_body, phase 4; specification: oracle/dexsim_oracle.c, "block-
// parallel projected Gauss-Seidel with mass splitting").  A lane's hand contacts are cut into runs of 2 consecutive list
// entries (of 4 when the lane has more than 12): run b is BLOCK b and belongs to wave b (0-5); the box/ground contacts are
// block 6 on the box wave.  In a sweep every block runs sequential projected Gauss-Seidel over its own contacts, all blocks
// at the same time, each on a private copy of the velocities in which a shared body (hand base, box, a finger whose contacts
// span two blocks) has 1/n of its mass; then the blocks' velocity changes are summed (exchange through LDS: FS_X, FS_T; two
// workgroup barriers per sweep).  The owner holds the 84 row words of each of its first two contacts in registers (HandRows)
// for all sweeps; only lanes with more than 12 hand contacts make a wave re-fetch rows inside the sweeps.
// (Round 2 first ran plain Gauss-Seidel in list order, handing the velocities from contact to contact across one barrier per
// pair of contacts: ~1.4k cycles per pair and sweep, sequential over ALL hand contacts of the lane.)
struct HandRows {
  f4 q[21];            // 3 rows x 7 quads: (t0..t3) (t4,t5,jf0,jf1) (jf2,jf3,St0,St1) (St2..St5) (Fj0..Fj3) (db,rxd0) (rxd1,rxd2,1/D,A)
  int kk;              // list entry (0 for lanes without the contact: every lane reads valid header / impulse words)
  bool act;
};
// The fetch of a contact's rows from the arena (crowq quad layout): 21 x 16 bytes per lane.  Addresses: scalar base + 32-bit
// lane offset; lanes without the contact read the always-zero quad row (entry KMAX, stride 0).
DI void hand_fetch(HandRows& R, const Arena& A, int j, int nbg, int nh, int N, int e) {
  R.act = j < nh;
  R.kk = R.act ? nbg + j : 0;
  const unsigned off0 = ((unsigned)((R.act ? R.kk : DEXSIM_KMAX) * 21) * (unsigned)N + (unsigned)e) * 16u;
  const unsigned stride = R.act ? (unsigned)N * 16u : 0u;
  const char* base = (const char*)A.crowq;   // wave-uniform: scalar base of the loads
#pragma unroll
  for (int q = 0; q < 21; q++) R.q[q] = *(const __attribute__((address_space(1))) f4*)(base + (off0 + (unsigned)q * stride));
}
// The shared velocity words (u_B, box twist) as packed pairs
struct TurnVel { f2 U01, U23, U45, V01, VW, W12; };
DI void turn_from_quads(TurnVel& v, f4 q0, f4 q1, f4 q2) { v.U01 = q0.xy; v.U23 = q0.zw; v.U45 = q1.xy; v.V01 = q1.zw; v.VW = q2.xy; v.W12 = q2.zw; }
// One projected Gauss-Seidel update of the contact in R inside its block: v = the block's copy of the shared velocities, G =
// its copy of the contact's finger velocities; nB, nF, the box's (nX / m, nX / I) = the split factors of the three bodies
// (the rows themselves are unsplit; 1/D and the in-contact couplings A_rs were built with the same factors).
DI void hand_update(const HandRows& R, TurnVel& v, f2& G01, f2& G23, f2 inv_mI_x, float nB, float nF, float mu, float cb, float (&lam)[3]) {
  // the three J.v products as three interleaved chains (written term by term: the row-by-row form is scheduled as one
  // 24-deep dependent chain of packed fmas, ~10 cycles each)
  const f4* q0 = R.q; const f4* q1 = R.q + 7; const f4* q2 = R.q + 14;
  f2 a0 = q0[0].xy * v.U01, a1 = q1[0].xy * v.U01, a2 = q2[0].xy * v.U01;
  a0 = q0[0].zw * v.U23 + a0; a1 = q1[0].zw * v.U23 + a1; a2 = q2[0].zw * v.U23 + a2;
  a0 = q0[1].xy * v.U45 + a0; a1 = q1[1].xy * v.U45 + a1; a2 = q2[1].xy * v.U45 + a2;
  a0 = q0[5].xy * v.V01 + a0; a1 = q1[5].xy * v.V01 + a1; a2 = q2[5].xy * v.V01 + a2;
  a0 = q0[5].zw * v.VW + a0; a1 = q1[5].zw * v.VW + a1; a2 = q2[5].zw * v.VW + a2;
  a0 = q0[6].xy * v.W12 + a0; a1 = q1[6].xy * v.W12 + a1; a2 = q2[6].xy * v.W12 + a2;
  a0 = q0[1].zw * G01 + a0; a1 = q1[1].zw * G01 + a1; a2 = q2[1].zw * G01 + a2;
  a0 = q0[2].xy * G23 + a0; a1 = q1[2].xy * G23 + a1; a2 = q2[2].xy * G23 + a2;
  float vr[3] = {a0.x + a0.y, a1.x + a1.y, a2.x + a2.y};
  const float A10 = R.q[6].w, A20 = R.q[13].w, A21 = R.q[20].w;
  const float nl0 = fmaxf(0.f, lam[0] - (vr[0] + cb) * R.q[6].z);
  const float dl0 = nl0 - lam[0], lim = mu * nl0;
  vr[1] += A10 * dl0; vr[2] += A20 * dl0;
  const float nl1 = clampf(lam[1] - vr[1] * R.q[13].z, -lim, lim);
  const float dl1 = nl1 - lam[1];
  vr[2] += A21 * dl1;
  const float nl2 = clampf(lam[2] - vr[2] * R.q[20].z, -lim, lim);
  const float dl2 = nl2 - lam[2];
  const float dl[3] = {dl0, dl1, dl2};
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const f4 *q = R.q + 7 * r;
    const float dB = nB * dl[r], dF = nF * dl[r];
    v.U01 = q[2].zw * dB + v.U01; v.U23 = q[3].xy * dB + v.U23; v.U45 = q[3].zw * dB + v.U45;
    G01 = q[4].xy * dF + G01; G23 = q[4].zw * dF + G23;
    const f2 dmI = inv_mI_x * dl[r];   // (nX dl/m, nX dl/I)
    v.V01 = q[5].xy * dmI.xx + v.V01; v.VW = q[5].zw * dmI + v.VW; v.W12 = q[6].xy * dmI.yy + v.W12;
  }
  lam[0] = nl0; lam[1] = nl1; lam[2] = nl2;
}
// warm start: the velocity change that goes with the contact's starting impulses, for the unsplit bodies
DI void hand_warm(const HandRows& R, TurnVel& v, f2& G01, f2& G23, f2 inv_mI, const float (&lam)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const f4 *q = R.q + 7 * r;
    v.U01 = q[2].zw * lam[r] + v.U01; v.U23 = q[3].xy * lam[r] + v.U23; v.U45 = q[3].zw * lam[r] + v.U45;
    G01 = q[4].xy * lam[r] + G01; G23 = q[4].zw * lam[r] + G23;
    const f2 dmI = inv_mI * lam[r];
    v.V01 = q[5].xy * dmI.xx + v.V01; v.VW = q[5].zw * dmI + v.VW; v.W12 = q[6].xy * dmI.yy + v.W12;
  }
}

// The row build of one work item's contact as a function of its own: every operand comes from LDS or the arena through this call's
// arguments, so that none of the builder's ~200 live values has to share a live range with the sweeps' state.  (Inlined like
// everything else here -- a real call would spill the caller's live values around it.)
DI void build_rows_item(const DevParams* __restrict__ P, int N, int ol, int k, int eo, int split, int gen) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  build_contact_rows<true>(P->arena, P, nullptr, sh, ol, k, N, eo, split, gen);
}

// ---- phases 3 and 4 of substep_body (general path: some hand contact in the workgroup) as a function of their own: everything the
// two phases need is in LDS and the arena, nothing of the caller's state is passed in registers -- their register need (84 row
// words per lane, the row builder's matrices) sits next to the few values substep_body keeps alive across them, not next to the
// finger dynamics' or the publication's.  (Inlined: the allocation is the whole kernel's, and it is close to the 256-register
// budget -- a change here is checked with -Rpass-analysis=kernel-resource-usage for 0 bytes of scratch.)
DI void general_contact_phases(const DevParams* __restrict__ P, int N, int wv, int lane, int e, const Stamps st, unsigned* probe) {
  extern __shared__ __attribute__((aligned(16))) float sh[];
  const Arena& A = P->arena;
  const DexSimConfig& C = P->cfg;
  const bool has_box = C.has_box != 0;
  float* s_uf = sh + FS_UF * 64;
  float* s_lam = sh + FS_LAM * 64;
  float* s_hdr = sh + FS_HDR * 64;
  int nc = __float_as_int(SH(DL_NC));
  const int nbg = (nc >> 8) & 0xff; nc &= 0xff;
  const int nh = nc - nbg;            // hand contacts of this lane
  int jmax = nh, kbg = nbg;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) { jmax = max(jmax, __shfl_xor(jmax, s)); kbg = max(kbg, __shfl_xor(kbg, s)); }
  jmax = __builtin_amdgcn_readfirstlane(jmax); kbg = __builtin_amdgcn_readfirstlane(kbg);
  // my place among the item processors: the finger waves first, the palm wave last.  (Round 2 first dealt the palm wave in as
  // the fourth, "to put the first four busy waves on four different SIMDs": but the palm wave shares its SIMD with the box
  // wave, which runs block 12 at raised priority, and it is also the heaviest reducer of the exchange -- its item phase took
  // 1.3k cycles against the finger waves' 0.8k and every pass waited for it.  Two item waves on one SIMD interleave for free.)
  // The box wave drops its raised priority for these phases: here it is one block among many, not the critical chain.
  // (Round 3 tried the palm wave as the fourth item wave once more -- the four busy waves of the settled regime on four different
  // SIMDs, with the reduction of u_B moved off the palm wave: 180 -> 190 us settled, like round 2's 178 -> 188.  The palm wave shares
  // SIMD 2 with the box wave's block 12; two finger waves on one SIMD interleave better than that pair.)
  if (wv == 6) __builtin_amdgcn_s_setprio(0);
  const int n_items = __builtin_amdgcn_readfirstlane(__float_as_int(sh[FS_NITEM * 64]));
  if (wv < 6) {
#pragma unroll 1
    for (int base = wv * 64; base < n_items; base += 6 * 64) {
      const int item = base + lane;
      if (item < n_items) {
        const int ent = __float_as_int(sh[FS_CTAB * 64 + item]);
        const int ol = ent & 0xff, blk = ent >> 8;   // owner lane, block
        const int nc_o = __float_as_int(sh[DL_NC * 64 + ol]), nbg_o = (nc_o >> 8) & 0xff, nh_o = (nc_o & 0xff) - nbg_o;
        const int split_o = __float_as_int(sh[FS_SPLIT * 64 + ol]), rs_o = SPLIT_RS(split_o);
#pragma unroll 1
        for (int c = 0; c <= rs_o; c++) {
          const int j = (blk << rs_o) + c;
          if (j < nh_o) build_rows_item(P, N, ol, nbg_o + j, blockIdx.x * 64 + ol, split_o, __float_as_int(sh[FS_GEN * 64 + ol]));
        }
      }
    }
  }
  st.mark<SG_BODY>(A, N, wv, e, PH_3_ROWS);   // phase 3 done
  __syncthreads();
  unsigned long long pr_t4 = 0;
  if (probe && wv == 0) pr_t4 = __builtin_amdgcn_s_memtime();

  // ---- phase 4: the block-parallel sweeps (see HandRows above).  Pass 0 applies the starting impulses (warm start), passes
  // 1 .. iters are the sweeps; every pass ends with the same exchange on all seven waves: barrier, the reducers (wave f: the
  // velocities of finger f; wave 5: u_B and box twist words 0-1; wave 6: box twist words 2-5) add the blocks' changes to the
  // common velocities of their own lane's env in block order, barrier.
  {
    const int iters = C.num_position_iterations;
    const bool bgstage = kbg > 0;           // wave-uniform: some lane has a box/ground contact
    const int split = __float_as_int(SH(FS_SPLIT)), gen = __float_as_int(SH(FS_GEN));
    float inv_m = 0.f, inv_I = 0.f;
    if (has_box) { inv_m = SH(FS_CMP_INVM); inv_I = SH(FS_CMP_INVM + 1); }
    const int nb_l = nh > 0 ? SPLIT_NB(split) : 0;    // hand blocks of this lane's env
    int nbmax = nb_l;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) nbmax = max(nbmax, __shfl_xor(nbmax, s));
    nbmax = __builtin_amdgcn_readfirstlane(nbmax);
    const float nXf = (float)SPLIT_NX(split), rX = 1.f / nXf;   // (the split factors 1/n stay on the operator: see schur_comp)
    if (wv == 6) {
      // the box wave: block 12 (box/ground contacts, all in VGPRs) + reducer of box twist words 2-5
      const int cpack = __float_as_int(SH(FS_CPACK));
      BoxBlock bb;
      bb.load<false>(kbg, inv_m, inv_I, s_lam, s_hdr, sh + FS_CMP * 64, 0, 0, lane, nbg, true, nXf);
      f4 Tm0 = *TQ(2);
      {
        f2 d01 = {0.f, 0.f}, d23 = {0.f, 0.f}, d45 = {0.f, 0.f};
        if (bgstage) bb.warm(d01, d23, d45, f2{inv_m, inv_I});
        *XQ(12, 1) = f4{0.f, 0.f, d01.x, d01.y}; *XQ(12, 2) = f4{d23.x, d23.y, d45.x, d45.y};
      }
#pragma unroll 1
      for (int it = 0; it <= iters; it++) {
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_WORK);
        __syncthreads();
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_BARRIER1);
        int b = 0;
        if (((nbmax + 3) & ~3) >= 8) {   // (eight blocks per batch, as on the palm wave)
          const f4 y0 = *XQ(0, 2), y1 = *XQ(1, 2), y2 = *XQ(2, 2), y3 = *XQ(3, 2), y4 = *XQ(4, 2), y5 = *XQ(5, 2), y6 = *XQ(6, 2), y7 = *XQ(7, 2);
          Tm0 += y0; Tm0 += y1; Tm0 += y2; Tm0 += y3; Tm0 += y4; Tm0 += y5; Tm0 += y6; Tm0 += y7;
          b = 8;
        }
#pragma unroll 1
        for (; b < ((nbmax + 3) & ~3); b += 4) {   // batches of four independent loads (unused blocks read as zero)
          const f4 y0 = *XQ(b, 2), y1 = *XQ(b + 1, 2), y2 = *XQ(b + 2, 2), y3 = *XQ(b + 3, 2);
          Tm0 += y0; Tm0 += y1; Tm0 += y2; Tm0 += y3;
        }
        Tm0 += *XQ(12, 2);
        *TQ(2) = Tm0;
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_REDUCED);
        __syncthreads();
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_BARRIER2);
        if (it == iters) break;
        if (it == 1) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_START);   // (the box block's work of pass 2 starts here)
        const f4 q1 = *TQ(1);
        const f2 o01 = q1.zw, o23 = Tm0.xy, o45 = Tm0.zw;
        f2 v01 = o01, v23 = o23, v45 = o45, d01 = {0.f, 0.f}, d23 = {0.f, 0.f}, d45 = {0.f, 0.f};
        if (bgstage) bb.sweep_delta(v01, v23, v45, d01, d23, d45, f2{inv_m, inv_I});
        *XQ(12, 1) = f4{0.f, 0.f, d01.x, d01.y}; *XQ(12, 2) = f4{d23.x, d23.y, d45.x, d45.y};
      }
      if (bgstage) { bb.store(s_lam, lane, nbg); cache_box_ground(A, s_lam, DEXSIM_WGEN_NEXT(gen), cpack, nbg, lane, N, e); }
      FLD(wgen, 0) = DEXSIM_WGEN_NEXT(gen);
      SH(FS_BOXV + 2) = Tm0.x; SH(FS_BOXV + 3) = Tm0.y; SH(FS_BOXV + 4) = Tm0.z; SH(FS_BOXV + 5) = Tm0.w;
    } else {
      // ---- reducer set-up (this lane's own env).  Finger wave f: the blocks of finger f are consecutive (list order); bit b of
      // q4mask = the finger's change sits in quad 4 of block b (second contact of a pair whose first contact is another finger's)
      const int rs_l = SPLIT_RS(split);
      int flo = 0, fcnt = 0, q4mask = 0;
      if (wv < 5) {
        int a = 0, cntf = 0;
#pragma unroll
        for (int w = 0; w < 5; w++) {
          const int word = NP_COUNT(__float_as_int(SH(FS_FLAG + w)));
          if (w < wv) a += word;
          if (w == wv) cntf = word;
        }
        cntf = max(0, min(cntf, nh - a));      // (list cut at KMAX)
        if (cntf > 0) {
          flo = a >> rs_l; fcnt = ((a + cntf - 1) >> rs_l) - flo + 1;
          if (rs_l && (a & 1)) q4mask = 1 << flo;   // the finger starts on the second contact of a pair
        }
      }
      int fcmax = fcnt;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) fcmax = max(fcmax, __shfl_xor(fcmax, s));
      fcmax = __builtin_amdgcn_readfirstlane(fcmax);
      // (the loads of a reduction are issued in one batch; blocks a lane's env does not have read as zero -- FS_X is cleared in
      // phase 3 -- so the sums need no per-lane masks; only the finger reducers, whose block range differs from lane to lane,
      // select)
      int it = 0;   // pass counter (profile stamps)
      const int nb4 = (nbmax + 3) & ~3;     // block loops run in batches of four independent loads (unused blocks read as zero)
      auto exchange = [&]() {
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_WORK);
        __syncthreads();
        if (it == 2) { st.mark<SG_SWEEP05>(A, N, wv, e, SW_BARRIER1); st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_BARRIER1); }
        if (wv < 5) {
          f4 t = *TQ(3 + wv);
#pragma unroll 1
          for (int i = 0; i < fcmax; i += 2) {
            const int b0 = min(flo + i, 11), b1 = min(flo + i + 1, 11);
            const f4 x0 = *XQ(b0, 3 + ((q4mask >> b0) & 1)), x1 = *XQ(b1, 3 + ((q4mask >> b1) & 1));
            if (i < fcnt) t += x0;
            if (i + 1 < fcnt) t += x1;
          }
          *TQ(3 + wv) = t;
        }
        // u_B and box twist words 0-1 (quads 0 and 1) on the palm wave, which takes items last.  (Round 3 tried one quad each on the
        // waves of fingers 3 and 4: those waves have items in the settled regime and their finger reduction in front of the quad --
        // 170 -> 181 us settled on the same box; quad 1 on the box wave 172 -> 176; quad 1 on the otherwise idle wave of finger 4
        // 171 -> 181: every variant that spreads the two quads loses.)
        if (wv == 5) {
          f4 t0 = *TQ(0);
          f4 t1 = *TQ(1);
          int b = 0;
          if (nb4 >= 8) {   // the first eight blocks in ONE batch of loads, same order of additions (171 -> 168 us settled: a batch of four per LDS round trip left the reducer waiting twice)
            const f4 y0 = *XQ(0, 0), y1 = *XQ(1, 0), y2 = *XQ(2, 0), y3 = *XQ(3, 0), y4 = *XQ(4, 0), y5 = *XQ(5, 0), y6 = *XQ(6, 0), y7 = *XQ(7, 0);
            const f4 z0 = *XQ(0, 1), z1 = *XQ(1, 1), z2 = *XQ(2, 1), z3 = *XQ(3, 1), z4 = *XQ(4, 1), z5 = *XQ(5, 1), z6 = *XQ(6, 1), z7 = *XQ(7, 1);
            t0 += y0; t0 += y1; t0 += y2; t0 += y3; t0 += y4; t0 += y5; t0 += y6; t0 += y7;
            t1 += z0; t1 += z1; t1 += z2; t1 += z3; t1 += z4; t1 += z5; t1 += z6; t1 += z7;
            b = 8;
          }
#pragma unroll 1
          for (; b < nb4; b += 4) {
            const f4 y0 = *XQ(b, 0), y1 = *XQ(b + 1, 0), y2 = *XQ(b + 2, 0), y3 = *XQ(b + 3, 0);
            const f4 z0 = *XQ(b, 1), z1 = *XQ(b + 1, 1), z2 = *XQ(b + 2, 1), z3 = *XQ(b + 3, 1);
            t0 += y0; t0 += y1; t0 += y2; t0 += y3;
            t1 += z0; t1 += z1; t1 += z2; t1 += z3;
          }
          *TQ(0) = t0;
          t1 += *XQ(12, 1);
          *TQ(1) = t1;
        }
        if (it == 2) { st.mark<SG_SWEEP05>(A, N, wv, e, SW_REDUCED); st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_REDUCED); }
        __syncthreads();
        if (it == 2) st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_BARRIER2);
      };
      const bool fast = jmax <= 12 && n_items <= 6 * 64;   // every block is one contact and every item has a lane of its own
      {
      // ---- my work item(s).  From here on `lane` / `e` name the OWNER's lane and env: all LDS words and arena rows of an item
      // belong to its owner.
      const int lane_phys = lane;
      if (fast) {
        // the common case: my item = ONE hand contact, resident in registers (rows, header, impulses) for all passes.  Per pass:
        // one batch of LDS reads (the common velocities), the update, the block's changes, the exchange.
        const bool have = wv * 64 + lane_phys < n_items;
        const int ent = have ? __float_as_int(sh[FS_CTAB * 64 + wv * 64 + lane_phys]) : lane_phys;
        const int lane = ent & 0xff, blk = ent >> 8, e = blockIdx.x * 64 + lane;
        const int nc_o = __float_as_int(SH(DL_NC)), nbg_o = (nc_o >> 8) & 0xff;
        const int split_o = __float_as_int(SH(FS_SPLIT)), gen_o = __float_as_int(SH(FS_GEN));
        const float nBo = (float)SPLIT_NB(split_o), nXo = (float)SPLIT_NX(split_o), rBo = 1.f / nBo, rXo = 1.f / nXo;
        const f2 inv_mI = {has_box ? SH(FS_CMP_INVM) : 0.f, has_box ? SH(FS_CMP_INVM + 1) : 0.f}, inv_mI_x = inv_mI * nXo;
        HandRows R;
        hand_fetch(R, A, have ? blk : DEXSIM_KMAX, nbg_o, have ? (nc_o & 0xff) - nbg_o : 0, N, e);
        const int kk = R.kk;
        const int code = __float_as_int(s_hdr[(4 * kk) * 64 + lane]), fo = __float_as_int(s_hdr[(4 * kk + 1) * 64 + lane]);
        const bool hasF = R.act && fo >= 0;
        const int qi = 3 + (max(fo, 0) >> 2);
        const float nFo = hasF ? (float)((code >> 12) & 15) : 0.f, rFo = hasF ? 1.f / nFo : 0.f;
        const float mu = R.act ? s_hdr[(4 * kk + 2) * 64 + lane] : 0.f, cb = R.act ? s_hdr[(4 * kk + 3) * 64 + lane] : 0.f;
        float lam[3];
#pragma unroll
        for (int r = 0; r < 3; r++) { const float l = s_lam[(3 * kk + r) * 64 + lane]; lam[r] = R.act ? l : 0.f; }
        // pass 0, warm start: the velocity changes that go with the starting impulses (unsplit bodies)
        if (have) {
          const f4 z4 = {0.f, 0.f, 0.f, 0.f};
          TurnVel vl;
          turn_from_quads(vl, z4, z4, z4);
          f2 G01 = z4.xy, G23 = z4.xy;
          hand_warm(R, vl, G01, G23, inv_mI, lam);
          *XQ(blk, 0) = f4{vl.U01.x, vl.U01.y, vl.U23.x, vl.U23.y}; *XQ(blk, 1) = f4{vl.U45.x, vl.U45.y, vl.V01.x, vl.V01.y};
          *XQ(blk, 2) = f4{vl.VW.x, vl.VW.y, vl.W12.x, vl.W12.y}; *XQ(blk, 3) = f4{G01.x, G01.y, G23.x, G23.y};
        }
        exchange();
#pragma unroll 1
        for (it = 1; it <= iters; it++) {
          if (it == 2) { st.mark<SG_SWEEP05>(A, N, wv, blockIdx.x * 64, SW_START); st.mark<SG_SWEEP_ALL>(A, N, wv, blockIdx.x * 64, SW_START); }
          if (have) {
            const f4 t0 = *TQ(0), t1 = *TQ(1), t2 = *TQ(2), tq = *TQ(qi);
            TurnVel vl;
            turn_from_quads(vl, t0, t1, t2);
            f2 G01 = tq.xy, G23 = tq.zw;
            hand_update(R, vl, G01, G23, inv_mI_x, nBo, nFo, mu, cb, lam);
            // my block's changes (for the unsplit bodies): local copy minus the common value it started from, over the split count
            const f2 dU01 = (vl.U01 - t0.xy) * rBo, dU23 = (vl.U23 - t0.zw) * rBo, dU45 = (vl.U45 - t1.xy) * rBo;
            const f2 dV01 = (vl.V01 - t1.zw) * rXo, dVW = (vl.VW - t2.xy) * rXo, dW12 = (vl.W12 - t2.zw) * rXo;
            const f2 dG01 = (G01 - tq.xy) * rFo, dG23 = (G23 - tq.zw) * rFo;
            *XQ(blk, 0) = f4{dU01.x, dU01.y, dU23.x, dU23.y}; *XQ(blk, 1) = f4{dU45.x, dU45.y, dV01.x, dV01.y};
            *XQ(blk, 2) = f4{dVW.x, dVW.y, dW12.x, dW12.y}; *XQ(blk, 3) = f4{dG01.x, dG01.y, dG23.x, dG23.y};
          }
          if (it == 2) st.mark<SG_SWEEP05>(A, N, wv, blockIdx.x * 64, SW_WORK);
          exchange();
          if (it == 2) st.mark<SG_SWEEP05>(A, N, wv, blockIdx.x * 64, SW_BARRIER2);
        }
        if (R.act) {   // impulses: to LDS (contact forces of the last sub-step) and to the warm-start cache
          s_lam[(3 * kk) * 64 + lane] = lam[0]; s_lam[(3 * kk + 1) * 64 + lane] = lam[1]; s_lam[(3 * kk + 2) * 64 + lane] = lam[2];
          st4_global(A.wlam + ((size_t)CODE_HKEY(code) * N + e) * 4, lam[0], lam[1], lam[2], __int_as_float(8 * DEXSIM_WGEN_NEXT(gen_o)));
        }
      } else {
        // ---- some lane has more than 12 hand contacts (its blocks are pairs) or there are more items than lanes: the items are
        // taken in rounds and the rows are fetched inside the passes; headers and impulses stay in LDS; within a pair one finger's
        // local velocities are carried from the first contact to the second.
        auto block_pass = [&](const bool warm) {
#pragma unroll 1
          for (int base = wv * 64; base < n_items; base += 6 * 64) {
            const bool have = base + lane_phys < n_items;
            const int ent = have ? __float_as_int(sh[FS_CTAB * 64 + base + lane_phys]) : lane_phys;
            const int lane = ent & 0xff, blk = ent >> 8, e = blockIdx.x * 64 + lane;
            const int nc_o = __float_as_int(SH(DL_NC)), nbg_o = (nc_o >> 8) & 0xff, nh_o = have ? (nc_o & 0xff) - nbg_o : 0;
            const int split_o = __float_as_int(SH(FS_SPLIT)), rs_o = SPLIT_RS(split_o);
            const float nBo = (float)SPLIT_NB(split_o), nXo = (float)SPLIT_NX(split_o);
            const f2 inv_mI = {has_box ? SH(FS_CMP_INVM) : 0.f, has_box ? SH(FS_CMP_INVM + 1) : 0.f}, inv_mI_x = inv_mI * nXo;
            const f4 z4 = {0.f, 0.f, 0.f, 0.f};
            TurnVel vl;
            if (warm) turn_from_quads(vl, z4, z4, z4); else turn_from_quads(vl, *TQ(0), *TQ(1), *TQ(2));
            int cur_fo = -1, cur_q = 3;
            float nFc = 1.f;
            f2 Gc01 = {0.f, 0.f}, Gc23 = {0.f, 0.f};
            auto flush = [&]() {
              if (cur_fo >= 0) {
                const f4 To = *TQ(3 + (cur_fo >> 2));
                const float rF = warm ? 1.f : 1.f / nFc;
                const f2 d01 = (Gc01 - (warm ? z4.xy : To.xy)) * rF, d23 = (Gc23 - (warm ? z4.zw : To.zw)) * rF;
                *XQ(blk, cur_q) = f4{d01.x, d01.y, d23.x, d23.y};
              }
            };
            HandRows R;
#pragma unroll 1
            for (int c = 0; c < (jmax > 12 ? 2 : 1); c++) {   // (second contacts exist only when some lane has pairs)
              hand_fetch(R, A, c <= rs_o ? (blk << rs_o) + c : DEXSIM_KMAX, nbg_o, nh_o, N, e);
              const int kk = R.kk;
              const int code = __float_as_int(s_hdr[(4 * kk) * 64 + lane]), fo = __float_as_int(s_hdr[(4 * kk + 1) * 64 + lane]);
              const float mu = R.act ? s_hdr[(4 * kk + 2) * 64 + lane] : 0.f, cb = R.act ? s_hdr[(4 * kk + 3) * 64 + lane] : 0.f;
              const bool hasF = R.act && fo >= 0;
              const f4 Tq = *TQ(3 + (max(fo, 0) >> 2));
              if (hasF && fo != cur_fo) {
                flush();
                Gc01 = warm ? z4.xy : Tq.xy; Gc23 = warm ? z4.zw : Tq.zw;
                cur_fo = fo; cur_q = 3 + c; nFc = (float)((code >> 12) & 15);
              }
              float lam[3];
#pragma unroll
              for (int r = 0; r < 3; r++) { const float l = s_lam[(3 * kk + r) * 64 + lane]; lam[r] = R.act ? l : 0.f; }
              if (warm) hand_warm(R, vl, Gc01, Gc23, inv_mI, lam);
              else {
                hand_update(R, vl, Gc01, Gc23, inv_mI_x, nBo, hasF ? nFc : 0.f, mu, cb, lam);
                if (R.act) { s_lam[(3 * kk) * 64 + lane] = lam[0]; s_lam[(3 * kk + 1) * 64 + lane] = lam[1]; s_lam[(3 * kk + 2) * 64 + lane] = lam[2]; }
              }
            }
            flush();
            if (have) {
              const float sB = warm ? 1.f : 1.f / nBo, sX = warm ? 1.f : 1.f / nXo;
              TurnVel vo;
              if (warm) turn_from_quads(vo, z4, z4, z4); else turn_from_quads(vo, *TQ(0), *TQ(1), *TQ(2));
              const f2 dU01 = (vl.U01 - vo.U01) * sB, dU23 = (vl.U23 - vo.U23) * sB, dU45 = (vl.U45 - vo.U45) * sB;
              const f2 dV01 = (vl.V01 - vo.V01) * sX, dVW = (vl.VW - vo.VW) * sX, dW12 = (vl.W12 - vo.W12) * sX;
              *XQ(blk, 0) = f4{dU01.x, dU01.y, dU23.x, dU23.y}; *XQ(blk, 1) = f4{dU45.x, dU45.y, dV01.x, dV01.y};
              *XQ(blk, 2) = f4{dVW.x, dVW.y, dW12.x, dW12.y};
              if (cur_fo < 0) *XQ(blk, 3) = z4;      // a block without a finger part: the reducers still read its quad 3
            }
          }
        };
#pragma unroll 1
        for (int it = 0; it <= iters; it++) {
          block_pass(it == 0);
          exchange();
        }
        // warm-start cache: the impulses my items' contacts end the sub-step with
#pragma unroll 1
        for (int base = wv * 64; base < n_items; base += 6 * 64) {
          if (base + lane_phys < n_items) {
            const int ent = __float_as_int(sh[FS_CTAB * 64 + base + lane_phys]);
            const int lane = ent & 0xff, blk = ent >> 8, e = blockIdx.x * 64 + lane;
            const int nc_o = __float_as_int(SH(DL_NC)), nbg_o = (nc_o >> 8) & 0xff, nh_o = (nc_o & 0xff) - nbg_o;
            const int rs_o = SPLIT_RS(__float_as_int(SH(FS_SPLIT))), gen_o = __float_as_int(SH(FS_GEN));
            for (int c = 0; c <= rs_o; c++) {
              const int j = (blk << rs_o) + c;
              if (j < nh_o) {
                const int kk = nbg_o + j;
                const int code = __float_as_int(s_hdr[(4 * kk) * 64 + lane]);
                st4_global(A.wlam + ((size_t)CODE_HKEY(code) * N + e) * 4, s_lam[(3 * kk) * 64 + lane], s_lam[(3 * kk + 1) * 64 + lane],
                           s_lam[(3 * kk + 2) * 64 + lane], __int_as_float(8 * DEXSIM_WGEN_NEXT(gen_o)));
              }
            }
          }
        }
      }
      }   // (owner's lane / env)
      // the common velocities go back to where phase 5 reads them
      if (wv < 5) {
        const f4 t = *TQ(3 + wv);
        s_uf[(4 * wv) * 64 + lane] = t.x; s_uf[(4 * wv + 1) * 64 + lane] = t.y; s_uf[(4 * wv + 2) * 64 + lane] = t.z;
        s_uf[(4 * wv + 3) * 64 + lane] = t.w;
      } else {
        const f4 t0 = *TQ(0), t1 = *TQ(1);
        SH(FS_UB) = t0.x; SH(FS_UB + 1) = t0.y; SH(FS_UB + 2) = t0.z; SH(FS_UB + 3) = t0.w; SH(FS_UB + 4) = t1.x; SH(FS_UB + 5) = t1.y;
        SH(FS_BOXV) = t1.z; SH(FS_BOXV + 1) = t1.w;
      }
    }
  }
  st.mark<SG_BODY>(A, N, wv, e, PH_4_SWEEPS);   // phase 4 done
  if (wv == 6) __builtin_amdgcn_s_setprio(2);
  __syncthreads();
  if (probe && wv == 0 && lane == 0) atomicAdd(probe + blockIdx.x * 4 + 3, (unsigned)(__builtin_amdgcn_s_memtime() - pr_t4));
}

// carry (k_physics4): what a body hands to the next inlined body without going through the arena -- the finger wave's own joint
// state in registers, base joints and box position (which every wave needs) through LDS words (FS_CARRY_*).  The arena is
// still written (publication, stand-alone stages); only the loads at the start of bodies 2-4, an L2 round trip behind the
// previous body's stores on every wave, go away.  carry_in: this body starts from the carried state; carry != nullptr: it
// leaves its end state behind (carry_out).
struct SubstepCarry { float ql[4], qdl[4], tg[4]; };
template <bool LAST, bool MS>
// seq: 1-based index of this body within the launch (token of the wave-5 -> wave-6 hand_free hand-off, see FS_FLAG)
// (st: the profiling build's cycle stamps of this body, dexsim_stamps.h)  post_pre (last sub-step of the fused control step only): the box wave, idle during the publication, already runs the
// post-physics tasks that do not depend on it (POST_PRE_MASK) into the observation tile at the bottom of the LDS
DI void substep_body(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int* __restrict__ cnt, int N, int NR, float* sh,
                     int seq, const Stamps st, bool post_pre, bool count_contacts, SubstepCarry& carry, bool carry_in, bool carry_out) {
  constexpr int dlb = FS_ROW;
  // contact statistics: only a control step's main physics step counts (a gated launch would race with finalize_stats);
  // word = stamp parity, see CNT_CONTACTS
  int* const ccnt = count_contacts ? cnt + (T.stamp & 1) : nullptr;
  constexpr int last = LAST ? 1 : 0;
  // (readfirstlane: the role is wave-uniform by construction; in an SGPR, everything indexed by it -- field rows f * 24 + i, LDS
  // words of finger f -- is scalar arithmetic instead of ~20 VGPRs of hoisted index products)
  const int wv = __builtin_amdgcn_readfirstlane(wave_role(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int e = blockIdx.x * 64 + lane;
  {
  const DexHandModel& M = P->model;
  const DexSimConfig& C = P->cfg;
  const float h = P->h;
  const V3 grav = v3p(C.gravity);
  const bool has_box = C.has_box != 0;
  float* s_uf = sh + FS_UF * 64;
  float* s_lam = sh + FS_LAM * 64;
  float* s_hdr = sh + FS_HDR * 64;
  // the box wave's chain (rows, then the sweeps) is long and it shares its SIMD with the light palm wave: let the SIMD's
  // arbiter prefer it
  if (wv == 6) __builtin_amdgcn_s_setprio(2);
  BaseChain B;
  FingerIn fin;
  // Two-level broadphase, one verdict per wave (LDS tokens FS_FLAG + w, w = finger 0-4 / palm 5): level 1 = bounding
  // sphere of the whole hand (hand_clear), known right after the base chain; level 2 = the per-capsule bounds, known
  // after the wave's own FK.  The box wave collects the six tokens before its contact solve; everybody else reads them
  // after the phase-1 barrier.  hand_free = all six clear.
  bool hand_free = false, sphere = false;
  V3 bpos_h = {0, 0, 0};
  M3 Rb_h = q2mat(Q4{0, 0, 0, 1});
  if (wv != 6) {   // the box wave needs neither the base chain nor the fingers: it starts on the box right away
    if (carry_in) {
      if (has_box) bpos_h = {SH(FS_CARRY_BP), SH(FS_CARRY_BP + 1), SH(FS_CARRY_BP + 2)};
      base_chain<MS>(A, P, grav, N, e, B, false, sh + FS_CARRY_Q * 64, sh + FS_CARRY_QD * 64, lane);
      if (wv < 5) {
#pragma unroll
        for (int l = 0; l < 4; l++) { fin.ql[l] = carry.ql[l]; fin.qdl[l] = carry.qdl[l]; fin.tg[l] = carry.tg[l]; }
      }
    } else {
      if (has_box) bpos_h = {FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2)};
      base_chain<MS>(A, P, grav, N, e, B, false);
      if (wv < 5) finger_load(A, wv, N, e, fin);
    }
    sphere = hand_clear(P, B, bpos_h);
    if (!sphere && has_box) Rb_h = q2mat(Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)});   // (capsule-level bounds: box frame)
    if (wv == 5) {
      bool pclear = sphere;
      if (!sphere) {
        const M3 R5 = q2mat(B.q5);
        bool clr = true;
#pragma unroll
        for (int cpl = 0; cpl < 3; cpl++)
          clr = clr && capsule_clear(B.o5 + mul(R5, v3p(M.cap_p0[cpl])), B.o5 + mul(R5, v3p(M.cap_p1[cpl])), M.cap_r[cpl], C, bpos_h, Rb_h);
        pclear = __all(clr);
      }
      if (lane == 0) sh[(FS_FLAG + 5) * 64] = __int_as_float((seq << 1) | (pclear ? 1 : 0));
    }
  }
  st.mark<SG_BODY>(A, N, wv, e, PH_BASE_CHAIN);

  // ---- phase 1
  int nc = 0, nbg = 0;
  float Gkeep[24];   // G_f of this finger wave, phase 1 -> phase 5 (see finger_dynamics; re-read from the arena when the hand is not clear)
#pragma unroll
  for (int i = 0; i < 24; i++) Gkeep[i] = 0.f;
  V3 bpos = {0, 0, 0}; M3 Rb = q2mat(Q4{0, 0, 0, 1});
  float hb = 0.f, bmu = 0.f;
  if (wv < 5) {
    finger_dynamics<MS>(A, P, B, fin, sh, dlb, s_uf, lane, wv, N, e, seq, sphere, bpos_h, Rb_h, Gkeep);
  } else if (wv == 5) {   // the palm
    const M3 R5 = q2mat(B.q5);
    Comp comp5;
    comp5.m = P->jc[5].mass;
    comp5.c = B.o5 + mul(R5, v3p(P->jc[5].com));
    comp5.I = rotate_inertia(R5, P->jc[5].inertia);
    V3 rc = comp5.c - B.o5;
    V3 ac = B.ao5 + cross(B.al5, rc) + cross(B.w5, cross(B.w5, rc));
    V3 f5 = comp5.m * ac;
    V3 n5 = mul(comp5.I, B.al5) + cross(B.w5, mul(comp5.I, B.w5)) + cross(rc, f5);
    comp_put(sh, lane, DL_PALM, comp5, B.o5);
    sh_put3(sh, lane, DL_PALM_WRENCH, f5); sh_put3(sh, lane, DL_PALM_WRENCH + 3, n5);
#pragma unroll
    for (int i = 0; i < 6; i++) SH(FS_TGTB + i) = FLD(targets, i);
#pragma unroll
    for (int i2 = 0; i2 < 3; i2++) {   // axes + origins of the base joints, two joints = 12 words = 3 quads (ROWADDR layout): row build (phase 3)
      const V3 a0 = B.ab[2 * i2], o0 = B.ob[2 * i2], a1 = B.ab[2 * i2 + 1], o1 = B.ob[2 * i2 + 1];
      *(f4*)(sh + FS_BCH * 64 + ROWADDR(12 * i2, lane)) = f4{a0.x, a0.y, a0.z, o0.x};
      *(f4*)(sh + FS_BCH * 64 + ROWADDR(12 * i2 + 4, lane)) = f4{o0.y, o0.z, a1.x, a1.y};
      *(f4*)(sh + FS_BCH * 64 + ROWADDR(12 * i2 + 8, lane)) = f4{a1.z, o1.x, o1.y, o1.z};
    }
    schur_precompute(sh, dlb, lane, B, seq, cnt);
  } else if (wv == 6) {   // the box: free velocity, box/ground contacts and their rows, (early mode) the contact solve
    float bv[6] = {0, 0, 0, 0, 0, 0};
    // warm-start cache of the box/ground contacts: one quad per LIST SLOT (80 + k: impulses, tag = 8 * generation + corner);
    // all four are fetched up front, next to the box state
    const int gen = FLD(wgen, 0);
    f4 wq[4];
#pragma unroll
    for (int k = 0; k < 4; k++) wq[k] = *(const __attribute__((address_space(1))) f4*)(A.wlam + ((size_t)(80 + k) * N + e) * 4);
    int cpack = 0;   // corner index of list slot k in bits [3k+2 : 3k]
    SH(FS_GEN) = __int_as_float(gen);
    if (has_box) {
      bpos = {FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2)};
      Rb = q2mat(Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)});
      hb = 0.5f * C.box_size;
      bmu = FLD(box_mu, 0);
      const float mu_bg = 0.5f * (bmu + C.ground_friction);
      const bool bfix = C.box_fixed != 0;   // the harness's static box: infinite mass, no gravity, no box/ground rows
      const float inv_m = bfix ? 0.f : rcp_n(FLD(box_mass, 0)) /* a body mass in kg */, inv_I = P->box_inv_I_k * inv_m;
      SH(FS_CMP_INVM) = inv_m; SH(FS_CMP_INVM + 1) = inv_I;
      V3 dirz[3];
      dirz[0] = v3(0, 0, 1);
      tangent_basis(dirz[0], dirz[1], dirz[2]);
      int k_unused = 0;   // running index of push_contact (== k at every call)
      // box/ground contacts: at most 4 (corner-index order), as compact rows (3 x 7 box words) + headers in LDS -- same
      // arithmetic as build_contact_rows for a type-2 contact.  Nothing here touches global memory: the manifold arrays /
      // force slots of these contacts are part of the observable state only after the LAST sub-step (below); the solver
      // reads the compact rows.  (Round 1 stored ~13 words per contact in every sub-step.)
#pragma unroll 1
      for (int i = 0; i < 8; i++) {
        V3 l = {(i & 1) ? hb : -hb, (i & 2) ? hb : -hb, (i & 4) ? hb : -hb};
        V3 p = mul(Rb, l) + bpos;
        if (!bfix && p.z < C.contact_offset && nc < 4) {
          const int k = nc++;
          cpack |= i << (3 * k);
          const float gap = p.z - C.rest_offset;
          const V3 rb = p - bpos;
          { float* rp = sh + (FS_CMP + 3 * k) * 64 + lane; rp[0] = rb.x; rp[64] = rb.y; rp[128] = rb.z; }
          const float cb = gap > 0.f ? div_n(gap, h) : -fminf(div_n(-gap * C.erp, h), C.max_depenetration_velocity);   // as in build_contact_rows
          s_hdr[(4 * k) * 64 + lane] = __int_as_float(2); s_hdr[(4 * k + 1) * 64 + lane] = __int_as_float(-1);
          s_hdr[(4 * k + 2) * 64 + lane] = mu_bg; s_hdr[(4 * k + 3) * 64 + lane] = cb;
          if (LAST) {   // observable after the step: manifold arrays, force slot / normal (solve_forces)
            push_contact(A, N, e, k_unused, 2, 0, i, p, dirz[0], gap, mu_bg, -1, nullptr, DEXSIM_FSLOT_BOX << 21);
            FLD(chdr, 8 * k + 4) = __int_as_float(DEXSIM_FSLOT_BOX);
            FLD(chdr, 8 * k + 5) = 0.f; FLD(chdr, 8 * k + 6) = 0.f; FLD(chdr, 8 * k + 7) = 1.f;
          }
        }
      }
      if (!bfix) {
        bv[0] = FLD(box_lin, 0) + h * grav.x; bv[1] = FLD(box_lin, 1) + h * grav.y; bv[2] = FLD(box_lin, 2) + h * grav.z;
        bv[3] = FLD(box_ang, 0); bv[4] = FLD(box_ang, 1); bv[5] = FLD(box_ang, 2);
      }
    }
    nbg = nc;
#pragma unroll
    for (int i = 0; i < 6; i++) SH(FS_BOXV + i) = bv[i];
    // starting impulses: the slot's cached ones if it held the same corner in the previous sub-step
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool warm = k < nc && __float_as_int(wq[k].w) == 8 * gen + ((cpack >> (3 * k)) & 7);
      s_lam[(3 * k) * 64 + lane] = warm ? wq[k].x : 0.f; s_lam[(3 * k + 1) * 64 + lane] = warm ? wq[k].y : 0.f;
      s_lam[(3 * k + 2) * 64 + lane] = warm ? wq[k].z : 0.f;
    }
    SH(FS_CPACK) = __int_as_float(cpack);   // for the box wave's general-path branch (phase 4)
    // SPECULATIVE box solve: the broadphase verdicts of the finger waves arrive only after their FK (~half of phase 1), and
    // in the regime that matters for throughput they say "hand clear".  So the box wave does not wait: it starts the sweeps
    // of the box/ground contacts right away, on a private copy of the twist in VGPRs, concurrently with the finger
    // dynamics, and commits the result (twist, impulses, forces) only if the hand turns out to be clear; otherwise the
    // result is dropped and the general path solves box/ground and hand contacts together from the free velocity, which is
    // still in FS_BOXV.  The block (rows, impulses, twist) stays in VGPRs across the phase-1 barrier; the last sweeps run
    // next to the Schur phase.  (Round 1 waited for the verdicts, swept 7 : 9 around the barrier and re-read the rows from
    // LDS behind it: the box wave was the last to reach both barriers, ~5k of a 43k-cycle sub-step.)
    BoxBlock sb;
    bool box_conv = false;   // (wave-uniform) a whole pass changed no impulse in any lane: the remaining passes are no-ops
    f2 sv01 = {bv[0], bv[1]}, sv23 = {bv[2], bv[3]}, sv45 = {bv[4], bv[5]};
    const int it_split = (C.num_position_iterations * SPEC_SPLIT_NUM) >> 4;   // sweeps next to the finger dynamics of phase 1
    const int tokw = (FS_FLAG + (lane < 6 ? lane : 0)) * 64;   // one token per lane: lane w < 6 reads wave w's, the others wave 0's again
    if (has_box) {
      int km = nc;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) km = max(km, __shfl_xor(km, s));
      sb.load<false>(km, SH(FS_CMP_INVM), SH(FS_CMP_INVM + 1), s_lam, s_hdr, sh + FS_CMP * 64, 0, 0, lane, nc, true);
      sb.warm(sv01, sv23, sv45, f2{SH(FS_CMP_INVM), SH(FS_CMP_INVM + 1)});
      // (the speculation is given up as soon as some wave has posted "not clear": in the contact regimes the 12 futile sweeps made the
      // box wave the last to reach the phase-1 barrier by ~2.7k cycles)
#pragma unroll 1
      for (int it = 0; it < it_split && !box_conv; it++) {
        // (the read is issued here and looked at behind the sweep, which works in VGPRs: the LDS round trip is off the sweep's path)
        const int tokv = lds_tok_load(sh, tokw);
        box_conv = !__any(sb.sweep(sv01, sv23, sv45));
        if (__any((tokv >> 1) == seq && !(tokv & 1))) break;
      }
    }
    {   // broadphase verdicts of this sub-step: the six tokens (fingers after their FK, palm after the base chain).
        // The spin is safe because the seven waves of a workgroup are always co-resident: a workgroup is placed on a CU as
        // a whole (448 threads = 7 waves, __launch_bounds__(448); FS_LDS_BYTES = 160 KiB of LDS => one workgroup per CU), and
        // the waves being waited for never wait for this one before they post their token.
        // One LDS read per poll: the six tokens in six lanes (tokw), a vote on "all posted", and the verdict is the AND of the
        // six clear bits of that same read.
      int tok;
      SPIN_GUARD_INIT();
      while (tok = lds_tok_load(sh, tokw), !__all((tok >> 1) == seq)) { __builtin_amdgcn_s_sleep(2); SPIN_GUARD(cnt, 2, seq); }
      hand_free = __all((tok & 1) != 0);
    }
    if (LAST && hand_free) FLD(ncontact, 0) = nc;
    SH(DL_NC) = __int_as_float(nc | (nbg << 8));
    // The box wave's own copy of the phase-1 barrier and of its phase 2 (the speculative block is only defined and used
    // inside this branch).
    st.mark<SG_BODY>(A, N, wv, e, PH_1);
    __syncthreads();
    if (hand_free) {   // the speculation held: the remaining sweeps, then commit twist, impulses and (last sub-step) forces
      if (has_box) {
#pragma unroll 1
        for (int it = it_split; it < C.num_position_iterations && !box_conv; it++) box_conv = !__any(sb.sweep(sv01, sv23, sv45));
        SH(FS_BOXV) = sv01.x; SH(FS_BOXV + 1) = sv01.y; SH(FS_BOXV + 2) = sv23.x; SH(FS_BOXV + 3) = sv23.y;
        SH(FS_BOXV + 4) = sv45.x; SH(FS_BOXV + 5) = sv45.y;
        sb.store(s_lam, lane);
        cache_box_ground(A, s_lam, DEXSIM_WGEN_NEXT(gen), cpack, nc, lane, N, e);
      }
      FLD(wgen, 0) = DEXSIM_WGEN_NEXT(gen);
      if (last) solve_forces_box(A, P, ccnt, s_lam, nc, lane, N, e, NR);   // (no box: nc = 0, clears the force slots)
    }
  }
  if (wv != 6) {
    st.mark<SG_BODY>(A, N, wv, e, PH_1);
    __syncthreads();
  }
  // Hand clear of box and ground in the whole workgroup and at most 4 box/ground contacts per env: the box and the
  // hand are dynamically decoupled in this sub-step, so wave 5 solves the box/ground contacts (rows it built itself in
  // phase 1) WHILE wave 0 reduces the Schur complement; phases 3 and 4 and their barriers disappear.
  // bit w: wave w's part of the hand cannot touch anything in this sub-step (one read, lane w < 6 of token w, and a ballot of bit 0)
  const int clear_mask = (int)(__ballot(lds_tok_load(sh, (FS_FLAG + (lane < 6 ? lane : 0)) * 64) & 1) & 63);
  hand_free = clear_mask == 63;
  const bool early = hand_free;

  // ---- phase 2
  float uB[6] = {0, 0, 0, 0, 0, 0};
  if (early && wv >= 1 && wv <= 3) {   // SCHUR_SPLIT: shares of the Schur phase on three of the waves that would wait at the barrier
    schur_helper(sh, dlb, wv - 1, lane);
    asm volatile("" ::: "memory");
    if (lane == 0) lds_tok_store(sh, (FS_FLAG + wv) * 64, (seq << 1) | 1 | SCHUR_SPLIT_BIT);   // a ds_write behind the data's ds_writes
  }
  if (wv == 0) {
    schur_base(A, P, B, sh, dlb, uB, lane, N, e, FS_TGTB, early, early ? seq : 0, st, cnt);
    if (early) {
#pragma unroll
      for (int i = 0; i < 6; i++) SH(FS_UB + i) = uB[i];
    }
  }
  if (!hand_free) {
    // Parallel narrowphase: wave f collides the capsules of finger f, wave 5 the palm's, each into its own staging block;
    // a finger (or the palm) whose capsules all passed their bounds is skipped.  Then the per-wave counts are exchanged
    // through LDS and every wave appends its contacts behind the box/ground ones in the oracle's fixed priority order
    // (finger 0..4 distal -> proximal, palm).  (Serial on one wave this was 75k of a 540k-cycle sub-step with all
    // fingers on the box.)
    int nloc = 0, tmask = 0;   // tmask: which of my local contacts are hand/box contacts
    // whose capsules this wave collides: its own -- except finger 0's, which the box wave takes (its speculative solve was
    // dropped, it idles here) so that wave 0 runs the Schur phase only: with both on wave 0 it set the length of phase 2
    const int cw = wv == 6 ? 0 : (wv == 0 ? -1 : wv);
    if (cw >= 0 && !((clear_mask >> cw) & 1)) {
      V3 bp = {0, 0, 0}; M3 Rbx = q2mat(Q4{0, 0, 0, 1});
      float hbx = 0.f, bmux = 0.f;
      if (has_box) {
        bp = wv == 6 ? bpos : bpos_h;
        Rbx = q2mat(Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)});
        hbx = 0.5f * C.box_size;
        bmux = FLD(box_mu, 0);
      }
      const float mu_hg = 0.5f * (M.hand_friction + C.ground_friction);
      const float mu_hb = 0.5f * (M.hand_friction + bmux);
      int caps[3], cinf[3];
      V3 E0[3], E1[3];
      float rr[3];
      if (cw < 5) {   // distal, middle, proximal
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const int l = 3 - c;
          caps[c] = 3 + 3 * cw + (l - 1);
          E0[c] = sh_get3(sh, lane, DL_CAPS(dlb, cw) + 6 * (l - 1)); E1[c] = sh_get3(sh, lane, DL_CAPS(dlb, cw) + 6 * (l - 1) + 3);
        }
      } else {
        const M3 R5 = q2mat(B.q5);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          caps[c] = c;
          E0[c] = B.o5 + mul(R5, v3p(M.cap_p0[c])); E1[c] = B.o5 + mul(R5, v3p(M.cap_p1[c]));
        }
      }
#pragma unroll
      for (int c = 0; c < 3; c++) { rr[c] = M.cap_r[caps[c]]; cinf[c] = code_info(M, caps[c]); }
      collide_capsules3(A, N, e, nloc, C, caps, E0, E1, rr, has_box, bp, Rbx, hbx, mu_hb, mu_hg, cw, &tmask, cinf);
    }
    const int nreal = nloc;
    if (C.joint_limit_rows && cw >= 0 && cw < 5 && __any(nreal > 0)) {
      // joint-limit rows of finger cw (oracle: push_limit_rows), behind the finger's contacts in its staging block, in the lanes
      // whose finger touches something: every joint within the margin of a limit, proximal to distal, lower before upper
      const bool touch = nreal > 0;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const int j = 6 + 4 * cw + l;
        const float qj = FLD(q, j);
        const float gl = qj - P->jc[j].lo, gu = P->jc[j].hi - qj;
        const int ci = ((cw + 1) << 16) | (l << 19);
        if (touch && gl < C.joint_limit_margin) push_contact(A, N, e, nloc, 3, l, 0, v3(0, 0, 0), v3(0, 0, 0), gl, 0.f, cw, nullptr, ci);
        if (touch && gu < C.joint_limit_margin) push_contact(A, N, e, nloc, 3, l, 1, v3(0, 0, 0), v3(0, 0, 0), gu, 0.f, cw, nullptr, ci);
      }
    }
    // counts (+ which contacts touch the box) go into the (now dead) token words, tagged so that they can never look like a
    // token of a later sub-step
    const int nbg0 = __float_as_int(SH(DL_NC)) & 0xff;   // box/ground contacts found by wave 6 (read before wave 0 rewrites the word)
    st.mark<SG_PH2>(A, N, wv, e, PH2_NARROW);
    if (cw >= 0) SH(FS_FLAG + cw) = __int_as_float(NP_TAG | ((clear_mask >> cw) & 1) | (nloc << 1) | (tmask << 8));
    __syncthreads();
    st.mark<SG_PH2>(A, N, wv, e, PH2_BARRIER);
    if (cw >= 0) {
      int off = nbg0;
      int tot = off;
#pragma unroll
      for (int w = 0; w < 6; w++) {
        const int c = NP_COUNT(__float_as_int(SH(FS_FLAG + w)));
        if (w < cw) off += c;
        tot += c;
      }
      // (four contacts per batch, all loads before the first store: one L2 round trip per batch -- contact by contact every
      // iteration waited for its own loads, ~1.5k cycles each, on the path of the phase-2 barrier)
#pragma unroll 1
      for (int i0 = 0; __any(i0 < nloc); i0 += 4) {
        f4 g0[4], g1[4];
        float gc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const bool ok = i0 + c < nloc && off + i0 + c < DEXSIM_KMAX;
          const int sc = cw * NP_STAGE + (ok ? i0 + c : 0);
          g0[c] = *FQ(cstage, 2 * sc); g1[c] = *FQ(cstage, 2 * sc + 1); gc[c] = FLD(cstage, CSTAGE_CODE0 + sc);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int kk = off + i0 + c;
          if (i0 + c < nloc && kk < DEXSIM_KMAX) {
            *FQ(cgeom, 2 * kk) = g0[c]; *FQ(cgeom, 2 * kk + 1) = g1[c];
            FLD(ccode, kk) = __float_as_int(gc[c]);
          }
        }
      }
      st.mark<SG_PH2>(A, N, wv, e, PH2_APPENDED);
    }
    if (wv == 0) {
      // list length, split counts and the work-item table: on wave 0, which has no capsules of its own to append (the box wave took
      // finger 0's) and would only wait at the barrier -- round 3 first had the palm wave do this BEHIND its own append, ~0.9k cycles
      // after every other wave had arrived
      int tot = nbg0;
#pragma unroll
      for (int w = 0; w < 6; w++) tot += NP_COUNT(__float_as_int(SH(FS_FLAG + w)));
      nc = min(tot, DEXSIM_KMAX);
      if (LAST) FLD(ncontact, 0) = nc;   // observable state only after the last sub-step; the kernel itself uses DL_NC
      SH(DL_NC) = __int_as_float(nc | (nbg0 << 8));
      // split counts of the block solver (see the oracle)
      int cntw[6], hmask = 0, o = nbg0;   // hmask: which hand contacts (by hand index) touch the box
#pragma unroll
      for (int w = 0; w < 6; w++) {
        const int word = __float_as_int(SH(FS_FLAG + w));
        const int c = NP_COUNT(word), eff = max(0, min(c, DEXSIM_KMAX - o)), a = min(o - nbg0, 31);
        cntw[w] = eff;
        hmask |= (NP_TMASK(word) & ((1 << eff) - 1)) << a;
        o += c;
      }
      const int split = split_pack(nbg0, cntw, hmask);
      SH(FS_SPLIT) = __int_as_float(split);
      // Work items.  Few lanes have many contacts, but a wave pays for its busiest lane: the row build and the sweeps therefore
      // do not run "lane = env" -- every hand BLOCK of the workgroup (= one hand contact; a pair in lanes with more than 12)
      // is an ITEM, and the items are dealt out densely over the lanes of waves 0-5 (table FS_CTAB: item -> owner lane, block).
      // The table is BLOCK-major: first every env's block 0, then every env's block 1, ...  Neighbouring item lanes then
      // belong to different envs, and their per-block LDS words ([word][owner lane]: headers, impulses, exchange quads) fall
      // into different banks; env-major, the blocks of one env sat side by side and collided on the owner's bank (6.5 % of the
      // wave cycles of the contact-rich regime were LDS bank conflicts).
      const int nh_l = nc - nbg0, nb_l = nh_l > 0 ? SPLIT_NB(split) : 0;
      float* ctab = sh + FS_CTAB * 64;
      int tot_items = 0;
#pragma unroll 1
      for (int b = 0; b < 12; b++) {
        const unsigned long long m = __ballot(b < nb_l);
        if (!m) break;
        if (b < nb_l) ctab[tot_items + __popcll(m & ((1ull << lane) - 1ull))] = __int_as_float(lane | (b << 8));
        tot_items += __popcll(m);
      }
      if (lane == 0) sh[FS_NITEM * 64] = __int_as_float(tot_items);
    }
  }
  st.mark<SG_BODY>(A, N, wv, e, PH_2);
  __syncthreads();

  // ---- phases 3 and 4 (general path): rows of the hand contacts, then the block-parallel sweeps -- general_contact_phases
  nc = __float_as_int(SH(DL_NC));
  nbg = (nc >> 8) & 0xff; nc &= 0xff;
  // Near, but nothing touches (round 3): some capsule failed its bounds, the narrowphase ran and found no hand contact in the whole
  // workgroup (a hand approaching its box spends many sub-steps within the bounds' ~4 cm before the first touch).  Hand and box are
  // then decoupled exactly as in the hand-clear case: wave 0 publishes u_B, the box wave solves the box/ground contacts alone -- the
  // early path's arithmetic (load, warm start, 16 sweeps in VGPRs) -- and phases 3-4 with their 17 x 2 barriers (~45k of a ~95k-cycle
  // sub-step, all of it exchange overhead around an empty item list) are skipped.
  const int n_items_wg = early ? 0 : __builtin_amdgcn_readfirstlane(__float_as_int(sh[FS_NITEM * 64]));
  const bool gp = !early && n_items_wg > 0;     // the general contact path proper
  if (!early && !gp) {
    if (wv == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) SH(FS_UB + i) = uB[i];
    } else if (wv == 6) {
      const int gen = __float_as_int(SH(FS_GEN)), cpack = __float_as_int(SH(FS_CPACK));
      if (has_box) {
        int km = nbg;
#pragma unroll
        for (int sf = 32; sf >= 1; sf >>= 1) km = max(km, __shfl_xor(km, sf));
        const f2 mI = {SH(FS_CMP_INVM), SH(FS_CMP_INVM + 1)};
        BoxBlock bb;
        f2 v01 = {SH(FS_BOXV), SH(FS_BOXV + 1)}, v23 = {SH(FS_BOXV + 2), SH(FS_BOXV + 3)}, v45 = {SH(FS_BOXV + 4), SH(FS_BOXV + 5)};
        bb.load<false>(km, mI.x, mI.y, s_lam, s_hdr, sh + FS_CMP * 64, 0, 0, lane, nbg, true);
        bb.warm(v01, v23, v45, mI);
#pragma unroll 1
        for (int it = 0; it < C.num_position_iterations; it++) if (!__any(bb.sweep(v01, v23, v45))) break;   // (fixed point: see BoxBlock::sweep)
        SH(FS_BOXV) = v01.x; SH(FS_BOXV + 1) = v01.y; SH(FS_BOXV + 2) = v23.x; SH(FS_BOXV + 3) = v23.y; SH(FS_BOXV + 4) = v45.x; SH(FS_BOXV + 5) = v45.y;
        bb.store(s_lam, lane);
        cache_box_ground(A, s_lam, DEXSIM_WGEN_NEXT(gen), cpack, nbg, lane, N, e);
      }
      FLD(wgen, 0) = DEXSIM_WGEN_NEXT(gen);
      if (last) solve_forces_box(A, P, ccnt, s_lam, nbg, lane, N, e, NR);
    }
    st.mark<SG_BODY>(A, N, wv, e, PH_3_ROWS); st.mark<SG_BODY>(A, N, wv, e, PH_4_SWEEPS);   // (phases 3 and 4 are empty on this path)
    __syncthreads();                // u_B and the box twist are read by every wave in phase 5
  }
  if (gp) {
  // the exchange words start at zero (blocks an env does not have must read as zero), the common velocities (FS_T) at the free
  // velocities
  {
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 10; q++) if (wv * 10 + q < 65) *XQ(0, wv * 10 + q) = z4;
    if (wv == 0) {
      *TQ(0) = f4{uB[0], uB[1], uB[2], uB[3]};
      float* t1 = (float*)TQ(1);
      t1[0] = uB[4]; t1[1] = uB[5];
    } else if (wv == 6) {
      float* t1 = (float*)TQ(1);
      t1[2] = SH(FS_BOXV); t1[3] = SH(FS_BOXV + 1);
      *TQ(2) = f4{SH(FS_BOXV + 2), SH(FS_BOXV + 3), SH(FS_BOXV + 4), SH(FS_BOXV + 5)};
    }
    if (wv < 5) *TQ(3 + wv) = f4{s_uf[(4 * wv) * 64 + lane], s_uf[(4 * wv + 1) * 64 + lane], s_uf[(4 * wv + 2) * 64 + lane], s_uf[(4 * wv + 3) * 64 + lane]};
  }
#pragma unroll
    for (int i = 0; i < 24; i++) Gkeep[i] = 0.f;   // (not live through phases 3-4: this path reads G_f back from the arena)
    unsigned long long pr_t3 = 0;
    if (T.probe && wv == 0) pr_t3 = __builtin_amdgcn_s_memtime();
    general_contact_phases(P, N, wv, lane, e, st, T.probe);
    if (T.probe && wv == 0 && lane == 0) {
      atomicAdd(T.probe + blockIdx.x * 4, (unsigned)(__builtin_amdgcn_s_memtime() - pr_t3));
      atomicAdd(T.probe + blockIdx.x * 4 + 2, 1u);
    }
  } else if (early) {
    st.mark<SG_BODY>(A, N, wv, e, PH_3_ROWS); st.mark<SG_BODY>(A, N, wv, e, PH_4_SWEEPS);   // (phases 3 and 4 are empty on this path)
  }

  // ---- phase 5: back-substitution qd = L^-1 u, semi-implicit Euler, joint-limit clamp; forces
  if (last && gp) {   // net contact forces of the general path: partial sums on waves 0-4 (the exchange words are dead: 5 x 51 rows)
    if (wv < 5) forces_partial(A, P, s_hdr, s_lam, sh + (FS_FORCE + wv * DEXSIM_NFSLOT * 3) * 64, nc, wv, lane, N, e);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 6; i++) uB[i] = SH(FS_UB + i);
  // (the joint-limit rows of the next body's narrowphase read q from the arena)
  const bool store_q = LAST || !carry_out || C.joint_limit_rows != 0;
  if (wv < 5) {
    const int f = wv;
    float G[24];   // all loads before the first q / qd store (see base_chain)
    if (sphere) {
#pragma unroll
      for (int i = 0; i < 24; i++) G[i] = Gkeep[i];
    } else {
#pragma unroll
      for (int qd = 0; qd < 6; qd++) { const f4 g4 = *FQ(fac_g, 6 * f + qd); G[4 * qd] = g4.x; G[4 * qd + 1] = g4.y; G[4 * qd + 2] = g4.z; G[4 * qd + 3] = g4.w; }
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
      float v = s_uf[(4 * f + l) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 6; i++) v -= G[l * 6 + i] * uB[i];
      float qn = 0.f, vn = 0.f;
      integrate_joint(A, P, h, 6 + 4 * f + l, fin.ql[l], v, N, e, &qn, &vn, store_q);
      if (carry_out) { carry.ql[l] = qn; carry.qdl[l] = vn; carry.tg[l] = fin.tg[l]; }
    }
  } else if (wv == 5) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float qn = 0.f, vn = 0.f;
      integrate_joint(A, P, h, i, B.qb[i], uB[i], N, e, &qn, &vn, store_q);
      if (carry_out) { SH(FS_CARRY_Q + i) = qn; SH(FS_CARRY_QD + i) = vn; }
    }
  } else {
    if (has_box) {
      float vb[3], wb[3];
#pragma unroll
      for (int i = 0; i < 3; i++) { vb[i] = SH(FS_BOXV + i); wb[i] = SH(FS_BOXV + 3 + i); }
      if (carry_out) { SH(FS_CARRY_BP) = fmaf(h, vb[0], bpos.x); SH(FS_CARRY_BP + 1) = fmaf(h, vb[1], bpos.y); SH(FS_CARRY_BP + 2) = fmaf(h, vb[2], bpos.z); }
      if (!C.box_fixed) integrate_box(A, h, vb, wb, N, e);   // (static box: its twist is exactly zero -- 1/m = 1/I = 0 in every row)
    }
  }
  if (last && wv < 5 && gp) forces_reduce(A, ccnt, s_hdr, sh + FS_FORCE * 64, nc, lane, N, e, NR, wv, 5);
  if (last && wv == 5 && gp) contact_stats(ccnt, s_hdr, nc, lane, e, NR);
  st.mark<SG_BODY>(A, N, wv, e, PH_5);
  }
  if (LAST) {
    __syncthreads();   // the publication reads the state written above by the other waves of the workgroup
    publish_body(A, T, P, 0, N, NR, 6);
    if (post_pre && wv == 6) post_pre_tasks(A, P, cnt, sh, N);
    st.mark<SG_BODY>(A, N, wv, e, PH_PUBLISH);
  }
}

DI void reset_phase1(const Arena& A, int N, int e);                                      // dexsim_l2.hip.inc
DI void finalize_stats(const ApiPtrs& T, const DevParams* __restrict__ P, int NR);
DI void post_block(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, int* __restrict__ cnt, float* s_ob,
                   int obs_only, int fold_reset, int N, int NR, int done_mask);
DI void actions_block(const Arena& A, const ApiPtrs& T, const DevParams* __restrict__ P, const float* __restrict__ act,
                      int zero_targets, int N, int NR);

// `tail` of a physics launch (host and kernels): what runs behind its last sub-step body
enum {
  TAIL_RESET = 1,       // gated launch: phase 1 of the in-step reset (after the extra physics step) + step statistics
  TAIL_POST = 2,        // ungated launch of dexsim_step: the whole post-physics block (observations, termination, rewards, phase 0
                        // of the in-step reset; k_post's body on the same 6 waves and the same LDS) runs right behind the last
                        // sub-step -- the state it reads is still in this CU's L1/L2 and one more kernel boundary disappears
  TAIL_NOT_FINAL = 4,   // not the last launch of a physics step: its last body does not add to the contact statistics
};

// The two ends that k_physics4 and k_physics1 share.  The big blocks between them -- actions_block, post_block -- are called by
// the kernels themselves: inlined through a helper of their own, they change k_physics4's code (post_block: 36 B of scratch).
// Prologue: start of the probe's launch time, the broadphase tokens (waves 0-5 -> wave 6, see substep_body).
template <bool GATED>
DI unsigned long long physics_prologue(const ApiPtrs& T, float* sh) {
  unsigned long long pr_k0 = 0;
  if (T.probe && threadIdx.x == 0) pr_k0 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x < 6) sh[(FS_FLAG + threadIdx.x) * 64] = 0.f;
  if (threadIdx.x == 6) sh[FS_COMPCNT * 64] = 0.f;
  return pr_k0;
}
// Epilogue: the gated launch closes the control step with the statistics of TerminationManager.evaluate (was k_finalize); the
// ungated one adds its launch time to the probe.
template <bool GATED>
DI void physics_epilogue(const ApiPtrs& T, const DevParams* __restrict__ P, int tail, unsigned long long pr_k0, int NR) {
  if (GATED && (tail & TAIL_RESET) && blockIdx.x == 0 && threadIdx.x == 0) finalize_stats(T, P, NR);
  if (!GATED && T.probe && threadIdx.x == 0) atomicAdd(T.probe + blockIdx.x * 4 + 1, (unsigned)(__builtin_amdgcn_s_memtime() - pr_k0));
}

// One sim.dt (4 sub-steps, the reference's and BASELINE's setting) in ONE launch: the four bodies are inlined back to
// back (straight-line code, no loop-carried registers -- unlike the rejected runtime loop), separated by workgroup
// barriers; envs are private to their workgroup, so no grid-wide ordering is needed.  Versus four launches this
// removes three kernel boundaries (~2.7 us each on this part: dispatch + the L2 writeback / invalidate that makes
// every first touch of the next kernel an Infinity-Cache / HBM miss, ~4k cycles).
// act != nullptr (ungated first launch of dexsim_step): ActionProcessor.process_actions runs first, three action channels per
// wavefront (actions_block, the body of k_actions too), so that the whole control step up to the reset gate is ONE launch.
// MS: the model has the structure of base_chain's specialised forms (classified by dexsim_create, which picks the kernel)
template <bool GATED, bool MS>
__global__ __launch_bounds__(448) void k_physics4(Arena A, ApiPtrs T, const DevParams* __restrict__ P, int* __restrict__ cnt,
                                                  const float* __restrict__ act, int tail, int N, int NR) {
  extern __shared__ float sh[];
  const unsigned long long pr_k0 = physics_prologue<GATED>(T, sh);
  if (!GATED && act) actions_block(P->arena, T, P, act, 0, N, NR);
  __syncthreads();   // targets are read by every wave of the first sub-step
  if (!GATED || cnt[CNT_ANY_RESET] == T.stamp) {
    SubstepCarry K;
    substep_body<false, MS>(P->arena, T, P, cnt, N, NR, sh, 1, Stamps::begin(1), false, true, K, false, true);
    __syncthreads();
    substep_body<false, MS>(P->arena, T, P, cnt, N, NR, sh, 2, Stamps::begin(2), false, true, K, true, true);
    __syncthreads();
    substep_body<false, MS>(P->arena, T, P, cnt, N, NR, sh, 3, Stamps::begin(3), false, true, K, true, true);
    __syncthreads();
    substep_body<true, MS>(P->arena, T, P, cnt, N, NR, sh, 4, Stamps::begin(4), !GATED && (tail & TAIL_POST), !GATED && !(tail & TAIL_NOT_FINAL), K, true, false);
    if (!GATED && (tail & TAIL_POST)) {
      __syncthreads();     // publication (site poses, hand twist) -> observations; LDS changes hands
      post_block(P->arena, T, P, cnt, sh, 0, 1, N, NR, POST_PRE_MASK);
    }
    if (GATED && (tail & TAIL_RESET)) {   // phase 1 of the in-step reset (after the extra physics step)
      const int e = blockIdx.x * 64 + (threadIdx.x & 63);
      if (threadIdx.x < 64 && e < NR && A.reset_flag[e] != 0) reset_phase1(A, N, e);
    }
  }
  physics_epilogue<GATED>(T, P, tail, pr_k0, NR);
}

// One sub-step in one launch, the same launch otherwise: the substeps % 4 sub-steps at the end of a physics step, and
// DEXSIM_STAGE_SUBSTEP.
template <bool GATED, bool MS>
__global__ __launch_bounds__(448) void k_physics1(Arena A, ApiPtrs T, const DevParams* __restrict__ P, int* __restrict__ cnt,
                                                  const float* __restrict__ act, int tail, int N, int NR) {
  extern __shared__ float sh[];
  const unsigned long long pr_k0 = physics_prologue<GATED>(T, sh);
  if (!GATED && act) actions_block(P->arena, T, P, act, 0, N, NR);
  __syncthreads();
  if (!GATED || cnt[CNT_ANY_RESET] == T.stamp) {
    SubstepCarry K;   // (a single body: nothing carried)
    substep_body<true, MS>(P->arena, T, P, cnt, N, NR, sh, 1, Stamps::begin(0), !GATED && (tail & TAIL_POST), !GATED && !(tail & TAIL_NOT_FINAL), K, false, false);
    if (!GATED && (tail & TAIL_POST)) {
      __syncthreads();
      post_block(P->arena, T, P, cnt, sh, 0, 1, N, NR, POST_PRE_MASK);
    }
    if (GATED && (tail & TAIL_RESET)) {
      const int e = blockIdx.x * 64 + (threadIdx.x & 63);
      if (threadIdx.x < 64 && e < NR && A.reset_flag[e] != 0) reset_phase1(A, N, e);
    }
  }
  physics_epilogue<GATED>(T, P, tail, pr_k0, NR);
}
