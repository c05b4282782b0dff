// dexsim_dynderiv.hip.inc -- derivatives of the inverse dynamics (dexsim_inverse_dynamics_derivatives, and the middle launch of
// dexsim_forward_dynamics_derivatives): d tau / d q and d tau / d qd of tau(q, qd, qdd) = M(q) qdd + c(q, qd) [+ g(q)], the function
// k_kin_invdyn computes, at fixed qdd.  Output rows are derivative-major: out[row, c, :] = d tau / d (q or qd)_c, 26 words.
//
// One kernel template, off the step path, in the workgroup of dexsim_chain.hip.inc (64 rows x 5 waves, lanes along the rows,
// [word][row] LDS, o5-relative positions).  The method is the tangent (forward mode) of k_kin_invdyn's Newton-Euler pass, one
// coordinate at a time.  A tangent carries, next to the derivative of the motion (w, al, ao), the virtual rotation th of the frame
// (d R = [th] x R): the axes, levers, centres and inertias of a frame turn with it, d a = th x a, d I = [th] I - I [th].
//
//   base pass c = 0 .. 5   every wave repeats the base chain's tangent and walks finger f: the finger's four torque tangents
//                          -> stage, its wrench tangent about o5 (and the wrench itself) -> LDS | wave 0 adds the palm link, sums
//                          the fingers in the order 0 .. 4 and projects on the six base joints, the derivative of the projection
//                          (axes and levers of the base joints) included | all waves flush the 26 words of row c
//   finger pass l = 0 .. 3 wave f differentiates by its own coordinate 6 + 4 f + l: the base does not move, so the wave projects
//                          its wrench tangent on the base joints itself; the other fingers' torques do not depend on the
//                          coordinate and are staged as +0.0 | all waves flush the five rows 6 + 4 ff + l
//
// Every pass walks the primal chain again next to its tangent (keeping four links' motions, wrenches, centres and inertias across
// the passes does not fit the registers), once for q and once for qd: POS = false has no virtual rotation and the compiler
// folds its terms away.  The two matrices share no arithmetic, so either one alone has the bits of both together.
//
// NEG stages the negated derivative (the right-hand sides of the forward route); the structural zeros stay +0.0.
//
// From dexsim_chain.hip.inc: the row rule (kd_load_q, kd_load_qd, kd_load_words for qdd), kd_base_walk, kd_finger_link, kd_flush
// (26 words into rows of 676).  From dexsim_invdyn.hip.inc: kd_joint_motion, kd_base_motion, kd_link_wrench.
//
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.

#define DD_WRP 0                                   /* [5][6] finger f's wrench about o5 */
#define DD_WRT (6 * DEXSIM_NFINGER)                /* [5][6] its tangent */
#define DD_ST (12 * DEXSIM_NFINGER)                /* [5][26] rows as they leave: base passes use the first */
#define DD_WORDS (DD_ST + DEXSIM_NFINGER * DEXSIM_NJ)
static_assert(DD_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_id_deriv: static LDS above 64 KiB");

struct IdDeriv {
  KinRows rows;
  const float* qd;     // (k, 26) override that goes with rows.q, or NULL = the arena's qd
  const float* qdd;    // (k, 26) aligned with the output rows, or NULL = zero
  float* dq;           // (k, 26, 26) or NULL
  float* dqd;          // (k, 26, 26) or NULL
  int gravity;         // DEXSIM_ID_GRAVITY
};

// One joint and its tangent along a direction whose component on this joint is s (of q if POS, else of qd): kd_joint_motion for
// m, and dm, the frame's virtual rotation th, d a and d r from the parent's (p, dp, thp).
template <bool POS>
DI void dd_joint(const KdMotion& p, const KdMotion& dp, V3 thp, V3 r, V3 a, float qd, float qdd, float s, bool slide, KdMotion& m,
                 KdMotion& dm, V3& th, V3& da, V3& dr) {
  const V3 wxa = cross(p.w, a);
  V3 dwxa = cross(dp.w, a);
  dm.ao = dp.ao + cross(dp.al, r) + cross(dp.w, cross(p.w, r)) + cross(p.w, cross(dp.w, r));
  if (POS) {
    da = cross(thp, a);
    dr = cross(thp, r);
    if (slide) dr += s * a;
    dm.ao += cross(p.al, dr) + cross(p.w, cross(p.w, dr));
    dwxa += cross(p.w, da);
  } else {
    da = v3(0, 0, 0);
    dr = v3(0, 0, 0);
  }
  const float dqd = POS ? 0.f : s;
  if (slide) {
    dm.w = dp.w; dm.al = dp.al; th = thp;
    dm.ao += (2.f * dqd) * wxa + (2.f * qd) * dwxa;
    if (POS) dm.ao += qdd * da;
  } else {
    dm.w = dp.w + dqd * a;
    dm.al = dp.al + dqd * wxa + qd * dwxa;
    th = thp;
    if (POS) { dm.w += qd * da; dm.al += qdd * da; th += s * a; }
  }
  m = kd_joint_motion(p, r, a, qd, qdd, slide);
}

// the base chain: kd_base_motion's walk with its tangent along the seed sb; d a and d orel of the six joints for the projection
template <bool POS>
DI void dd_base(const KinBase& B, const float* vb, const float* ab, V3 a0, const float* sb, KdMotion& m5, KdMotion& dm5, V3& th5,
                V3* da, V3* dorel) {
  KdMotion m = {v3(0, 0, 0), v3(0, 0, 0), a0}, dm = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};
  V3 th = v3(0, 0, 0), dr[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const V3 r = j == 0 ? v3(0, 0, 0) : B.orel[j] - B.orel[j - 1];
    KdMotion mn, dmn;
    V3 thn;
    dd_joint<POS>(m, dm, th, r, B.a[j], vb[j], ab[j], sb[j], j < 3, mn, dmn, thn, da[j], dr[j]);
    m = mn; dm = dmn; th = thn;
  }
  dorel[5] = v3(0, 0, 0);
#pragma unroll
  for (int j = 4; j >= 0; j--) dorel[j] = dorel[j + 1] - dr[j + 1];
  m5 = m; dm5 = dm; th5 = th;
}

// tangent of kd_link_wrench: the link's frame has the motion m, its tangent dm and the virtual rotation th; f is the link's force
template <bool POS>
DI void dd_link_wrench(float mass, V3 rc, const S6& I, const KdMotion& m, const KdMotion& dm, V3 th, V3 f, V3& df, V3& dn) {
  V3 dac = dm.ao + cross(dm.al, rc) + cross(dm.w, cross(m.w, rc)) + cross(m.w, cross(dm.w, rc));
  const V3 Iw = mul(I, m.w);
  dn = mul(I, dm.al) + cross(dm.w, Iw) + cross(m.w, mul(I, dm.w));
  if (POS) {
    const V3 drc = cross(th, rc);
    dac += cross(m.al, drc) + cross(m.w, cross(m.w, drc));
    dn += cross(th, mul(I, m.al)) - mul(I, cross(th, m.al));                  // d I al
    dn += cross(m.w, cross(th, Iw) - mul(I, cross(th, m.w)));                 // w x d I w
    dn += cross(drc, f);
  }
  df = mass * dac;
  dn += cross(rc, df);
}

// Finger f below the palm frame (m5, dm5, th5), tangent along the seed sf of its own joints: the torque tangents dt[4], the wrench
// about o5 (F, Nm) and its tangent (dF, dN).
template <bool POS>
DI void dd_finger(const DevParams* __restrict__ P, int f, Q4 q5, const float* qf, const float* vf, const float* af, const KdMotion& m5,
                  const KdMotion& dm5, V3 th5, const float* sf, float* dt, V3& F, V3& Nm, V3& dF, V3& dN) {
  V3 a[4], r[4], fl[4], nl[4], dfl[4], dnl[4];
  V3 th = th5;
  {
    V3 of = v3(0, 0, 0), op = v3(0, 0, 0);
    Q4 qc = q5;
    KdMotion m = m5, dm = dm5;
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const JC& c = P->jc[6 + 4 * f + l];
      V3 rc, thn, da, dr;
      S6 I;
      KdMotion mn, dmn;
      kd_finger_link(c, qf[l], of, qc, a[l], rc, I);
      r[l] = of - op;
      op = of;
      dd_joint<POS>(m, dm, th, r[l], a[l], vf[l], af[l], sf[l], false, mn, dmn, thn, da, dr);
      m = mn; dm = dmn; th = thn;
      kd_link_wrench(c.mass, rc, I, m, fl[l], nl[l]);
      dd_link_wrench<POS>(c.mass, rc, I, m, dm, th, fl[l], dfl[l], dnl[l]);
      __builtin_amdgcn_sched_barrier(0);   // link by link, as k_kin_fwddyn: four links' inertias and tangents do not fit the registers
    }
  }
  // backward: d a_l = thp_l x a_l and d r_l = thp_l x r_l with thp_l the virtual rotation of joint l's parent, unwound from the
  // last frame's (exact: a seed is 0 or 1 and only one is set) instead of kept per link
  F = fl[3]; Nm = nl[3]; dF = dfl[3]; dN = dnl[3];
  dt[3] = dot(a[3], dN);
  if (POS) { th -= sf[3] * a[3]; dt[3] += dot(cross(th, a[3]), Nm); }
#pragma unroll
  for (int l = DEXSIM_NFJ - 2; l >= 0; l--) {
    dN = dnl[l] + dN + cross(r[l + 1], dF);
    if (POS) { dN += cross(cross(th, r[l + 1]), F); th -= sf[l] * a[l]; }
    Nm = nl[l] + Nm + cross(r[l + 1], F);
    F = fl[l] + F;
    dF = dfl[l] + dF;
    dt[l] = dot(a[l], dN);
    if (POS) dt[l] += dot(cross(th, a[l]), Nm);
  }
  dN = dN + cross(r[0], dF);   // about o5
  if (POS) dN += cross(cross(th5, r[0]), F);
  Nm = Nm + cross(r[0], F);
}

// What a pass reads of the row.  Every pass starts from a copy whose origin the optimiser does not see (dd_fresh: no instruction):
// otherwise it hoists whatever does not depend on the pass -- the whole primal walk -- out of the loops and keeps four links'
// motions, wrenches, centres and inertias in registers across them.
struct DdRow { KinBase B; float qf[4], vb[6], vf[4], ab[6], af[4]; V3 a0; };

DI V3 dd_fresh(V3 v) { return {opaque(v.x), opaque(v.y), opaque(v.z)}; }
DI DdRow dd_fresh(const DdRow& R) {
  DdRow O;
#pragma unroll
  for (int j = 0; j < 6; j++) { O.B.a[j] = dd_fresh(R.B.a[j]); O.B.orel[j] = dd_fresh(R.B.orel[j]); O.vb[j] = opaque(R.vb[j]); O.ab[j] = opaque(R.ab[j]); }
#pragma unroll
  for (int l = 0; l < DEXSIM_NFJ; l++) { O.qf[l] = opaque(R.qf[l]); O.vf[l] = opaque(R.vf[l]); O.af[l] = opaque(R.af[l]); }
  O.B.q[5] = {opaque(R.B.q[5].x), opaque(R.B.q[5].y), opaque(R.B.q[5].z), opaque(R.B.q[5].w)};
  O.a0 = dd_fresh(R.a0);
  return O;
}

// base pass: row c (a base coordinate) of one matrix
template <bool POS, bool NEG>
DI void dd_base_pass(const DevParams* __restrict__ P, const DdRow& row, int c, float* out, float* s_w, const int* s_valid, int lane, int f) {
  const float sg = NEG ? -1.f : 1.f;
  float sb[6];
#pragma unroll
  for (int j = 0; j < 6; j++) sb[j] = c == j ? 1.f : 0.f;
  const float sf[4] = {0.f, 0.f, 0.f, 0.f};
  {
    const DdRow R = dd_fresh(row);
    KdMotion m5, dm5;
    V3 th5, da[6], dorel[6];
    dd_base<POS>(R.B, R.vb, R.ab, R.a0, sb, m5, dm5, th5, da, dorel);
    float dt[4];
    V3 F, Nm, dF, dN;
    dd_finger<POS>(P, f, R.B.q[5], R.qf, R.vf, R.af, m5, dm5, th5, sf, dt, F, Nm, dF, dN);
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) s_w[(DD_ST + 6 + 4 * f + l) * KD_LD + lane] = sg * dt[l];
    KD_PUT3(DD_WRT + 6 * f, dF);
    KD_PUT3(DD_WRT + 6 * f + 3, dN);
    if (POS) { KD_PUT3(DD_WRP + 6 * f, F); KD_PUT3(DD_WRP + 6 * f + 3, Nm); }
  }
  __syncthreads();
  if (f == 0) {   // the palm link and the five fingers, projected on the six base joints
    // the base tangent once more, from a fresh copy again: kept across the finger walk its 57 words (motion, tangent, d a,
    // d orel) spill
    const DdRow R = dd_fresh(row);
    const KinBase& B = R.B;
    KdMotion m5, dm5;
    V3 th5, da[6], dorel[6];
    dd_base<POS>(B, R.vb, R.ab, R.a0, sb, m5, dm5, th5, da, dorel);
    const JC& c5 = P->jc[5];
    const M3 R5 = q2mat(B.q[5]);
    const V3 rc = mul(R5, v3p(c5.com));
    const S6 I = rotate_inertia(R5, c5.inertia);
    V3 F, Nm, dF, dN;
    kd_link_wrench(c5.mass, rc, I, m5, F, Nm);
    dd_link_wrench<POS>(c5.mass, rc, I, m5, dm5, th5, F, dF, dN);
#pragma unroll
    for (int ff = 0; ff < DEXSIM_NFINGER; ff++) {
      const float* const w = s_w + (DD_WRT + 6 * ff) * KD_LD + lane;
      dF += v3(w[0], w[KD_LD], w[2 * KD_LD]);
      dN += v3(w[3 * KD_LD], w[4 * KD_LD], w[5 * KD_LD]);
      if (POS) {
        const float* const p = s_w + (DD_WRP + 6 * ff) * KD_LD + lane;
        F += v3(p[0], p[KD_LD], p[2 * KD_LD]);
        Nm += v3(p[3 * KD_LD], p[4 * KD_LD], p[5 * KD_LD]);
      }
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {   // the moment about o_j: o5 - o_j = -orel[j]
      float t;
      if (j < 3) {
        t = dot(B.a[j], dF);
        if (POS) t += dot(da[j], F);
      } else {
        V3 dM = dN - cross(B.orel[j], dF);
        if (POS) dM -= cross(dorel[j], F);
        t = dot(B.a[j], dM);
        if (POS) t += dot(da[j], Nm - cross(B.orel[j], F));
      }
      s_w[(DD_ST + j) * KD_LD + lane] = sg * t;
    }
  }
  __syncthreads();
  kd_flush<false>(s_w, s_valid, DD_ST, DEXSIM_NJ, out, (size_t)DEXSIM_NJ * DEXSIM_NJ, (size_t)DEXSIM_NJ * c);
  __syncthreads();   // the next pass stages over these words
}

// finger pass: rows 6 + 4 ff + l (joint l of every finger) of one matrix
template <bool POS, bool NEG>
DI void dd_finger_pass(const DevParams* __restrict__ P, const DdRow& row, int l0, float* out, float* s_w, const int* s_valid, int lane, int f) {
  const float sg = NEG ? -1.f : 1.f;
  float sf[4];
#pragma unroll
  for (int l = 0; l < DEXSIM_NFJ; l++) sf[l] = l0 == l ? 1.f : 0.f;
  const DdRow R = dd_fresh(row);
  const KinBase& B = R.B;
  KdMotion mb[6];
  kd_base_motion(B, R.vb, R.ab, R.a0, mb);
  float dt[4];
  V3 F, Nm, dF, dN;
  const KdMotion z = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};   // the palm frame does not move with a finger's coordinate
  dd_finger<POS>(P, f, B.q[5], R.qf, R.vf, R.af, mb[5], z, v3(0, 0, 0), sf, dt, F, Nm, dF, dN);
  float* const st = s_w + (DD_ST + DEXSIM_NJ * f) * KD_LD + lane;
#pragma unroll
  for (int j = 0; j < 6; j++)   // the base joints' axes and levers do not depend on a finger's coordinate
    st[j * KD_LD] = sg * (j < 3 ? dot(B.a[j], dF) : dot(B.a[j], dN - cross(B.orel[j], dF)));
#pragma unroll
  for (int ff = 0; ff < DEXSIM_NFINGER; ff++)
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) st[(6 + 4 * ff + l) * KD_LD] = ff == f ? sg * dt[l] : 0.f;
  __syncthreads();
  for (int ff = 0; ff < DEXSIM_NFINGER; ff++)
    kd_flush<false>(s_w, s_valid, DD_ST + DEXSIM_NJ * ff, DEXSIM_NJ, out, (size_t)DEXSIM_NJ * DEXSIM_NJ, (size_t)DEXSIM_NJ * (6 + 4 * ff + l0));
  __syncthreads();   // the next pass stages over these words
}

template <bool NEG>
__global__ __launch_bounds__(KD_THREADS) void k_kin_id_deriv(const DevParams* __restrict__ P, IdDeriv K, int N, int NR) {
  __shared__ float s_w[DD_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;

  DdRow R;
  float qb[6];
  const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, R.qf);
  kd_load_qd(A, K.rows, K.qd, N, NR, f, R.vb, R.vf);
#pragma unroll
  for (int j = 0; j < 6; j++) R.ab[j] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++) R.af[j] = 0.f;
  if (K.qdd) kd_load_words(K.qdd, (size_t)kd_row(K.rows) * DEXSIM_NJ, 1, f, R.ab, R.af);
  kd_base_walk(P, qb, R.B);
  if (f == 0) s_valid[lane] = valid;
  const V3 g = v3p(P->cfg.gravity);
  R.a0 = K.gravity ? v3(-g.x, -g.y, -g.z) : v3(0, 0, 0);

#pragma unroll 1
  for (int c = 0; c < 6; c++) {
    if (K.dq) dd_base_pass<true, NEG>(P, R, c, K.dq, s_w, s_valid, lane, f);
    if (K.dqd) dd_base_pass<false, NEG>(P, R, c, K.dqd, s_w, s_valid, lane, f);
  }
#pragma unroll 1
  for (int l0 = 0; l0 < DEXSIM_NFJ; l0++) {
    if (K.dq) dd_finger_pass<true, NEG>(P, R, l0, K.dq, s_w, s_valid, lane, f);
    if (K.dqd) dd_finger_pass<false, NEG>(P, R, l0, K.dqd, s_w, s_valid, lane, f);
  }
}
