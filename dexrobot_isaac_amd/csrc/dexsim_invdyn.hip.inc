// dexsim_invdyn.hip.inc -- inverse dynamics and bias accelerations of the hand (dexsim_inverse_dynamics, dexsim_body_bias_accel):
// tau = M(q) qdd + c(q, qd) [+ g(q)] and Jdot qd of the published hand bodies, functions of (q, qd) with the M, c and g of
// dexsim_mass_matrix -- general symmetric link inertias, no armature, no PD, no contact, no joint-limit terms.
//
// Two kernels, neither on the step path; both read q and qd (arena rows or the caller's overrides) and write caller-owned memory
// only, in the workgroup of dexsim_chain.hip.inc (64 rows x 5 waves, lanes along the rows, [word][row] LDS, o5-relative positions).
// Both are a recursive Newton-Euler walk in world axes; the state of a frame is (w, al, ao): angular velocity, angular acceleration
// and the CLASSICAL acceleration of the frame's origin (d/dt of its velocity), so gravity is the base acceleration -g.
//
//   k_kin_invdyn      forward  every wave repeats the base chain (kd_base_walk), then walks its finger; each link's wrench about its
//                              frame origin (f = m a_c, n = I al + w x I w + rc x f) is formed on the way down
//                     backward over the finger's four links: the finger joints' torques, and the finger's wrench about o5 -> LDS
//                     palm     after one __syncthreads(), wave 0 adds the palm link and the five finger wrenches and projects the
//                              sum on the six base joints: links 0-4 are massless (validate_model), so every base joint carries the
//                              whole hand, exactly as k_kin_mass treats them
//   k_kin_bias_accel  the forward pass alone at qdd = 0 and without gravity, then a_b = ao + al x r + w x (w x r) and al for the
//                     requested bodies welded to each joint frame (kd_body_joint; the host sorts the request by frame): 6 words per body
//
// From dexsim_chain.hip.inc: the row rule (kd_load_q, kd_load_qd, kd_load_words for qdd), kd_base_walk, the link walk kd_finger_link
// (k_kin_bias_accel needs no centre or inertia and walks kd_finger_joint), kd_flush.  The Newton-Euler set defined here --
// kd_joint_motion, kd_link_wrench, kd_finger_backward, kd_palm_project -- is also k_kin_fwddyn<true>'s (dexsim_fwddyn.hip.inc);
// k_kin_invdyn spells the last two out (see there).
//
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.
// Numerics: only differences of o5-relative origins enter (levers of hand size); the spawn position never does -- joint 0 hangs
// on a frame that neither turns nor accelerates, so its lever drops out.

#define ID_TAU 0                                   /* [26] joint forces, as they leave */
#define ID_WR DEXSIM_NJ                            /* [5][6] finger f's wrench about o5: force, moment */
#define ID_WORDS (ID_WR + 6 * DEXSIM_NFINGER)
#define BA_WORDS (6 * DEXSIM_NUM_HAND_BODIES)      /* [nb][6]: linear, angular */
static_assert(ID_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_invdyn: static LDS above 64 KiB");
static_assert(BA_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_bias_accel: static LDS above 64 KiB");

struct InvDyn {
  KinRows rows;
  const float* qd;     // (k, 26) override that goes with rows.q, or NULL = the arena's qd
  const float* qdd;    // (k, 26) aligned with the output rows, or NULL = zero
  float* tau;          // (k, 26)
  int gravity;         // DEXSIM_ID_GRAVITY
};

struct BiasAcc {
  KinRows rows;
  const float* qd;
  float* acc;                                       // (k, nb, 6)
  int nb;
  // the nb requested bodies sorted by the frame they ride on (host side), so that a wave visits its own bodies only: entries
  // [jstart[j + 1], jstart[j + 2]) ride on joint frame j (j = -1: the fixed spawn frame); entry i is body body[i], output slot slot[i]
  unsigned char body[DEXSIM_NUM_HAND_BODIES + 3], slot[DEXSIM_NUM_HAND_BODIES + 3];
  unsigned char jstart[DEXSIM_NJ + 2];
};

struct KdMotion { V3 w, al, ao; };

// One joint: the parent frame's motion -> this frame's.  r = o_j - o_parent (a slide's displacement included), a the world axis.
// ao first becomes the acceleration of the point of the PARENT that coincides with o_j; a slide adds the Coriolis term and its own
// acceleration along the axis, a hinge turns w and al.
DI KdMotion kd_joint_motion(const KdMotion& p, V3 r, V3 a, float qd, float qdd, bool slide) {
  KdMotion m;
  m.ao = p.ao + cross(p.al, r) + cross(p.w, cross(p.w, r));
  const V3 wxa = cross(p.w, a);
  if (slide) { m.w = p.w; m.al = p.al; m.ao += (2.f * qd) * wxa + qdd * a; }
  else { m.w = p.w + qd * a; m.al = p.al + qd * wxa + qdd * a; }
  return m;
}

// classical acceleration of the point at r from the frame's origin, fixed in the frame
DI V3 kd_point_accel(const KdMotion& m, V3 r) { return m.ao + cross(m.al, r) + cross(m.w, cross(m.w, r)); }

// the six base joints; a0 = the acceleration of the fixed spawn frame (-g, or zero).  Joint 0's lever never counts: its parent
// neither turns nor has an angular acceleration.
// ab == nullptr: no joint accelerations.
DI void kd_base_motion(const KinBase& B, const float* vb, const float* ab, V3 a0, KdMotion* mb) {
  KdMotion m = {v3(0, 0, 0), v3(0, 0, 0), a0};
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const V3 r = j == 0 ? v3(0, 0, 0) : B.orel[j] - B.orel[j - 1];
    m = kd_joint_motion(m, r, B.a[j], vb[j], ab ? ab[j] : 0.f, j < 3);
    mb[j] = m;
  }
}

// the wrench a link (mass, centre rc from its frame's origin, inertia I in world axes) needs, about that origin: f = m a_c,
// n = I al + w x (I w) + rc x f
DI void kd_link_wrench(float mass, V3 rc, const S6& I, const KdMotion& m, V3& f, V3& n) {
  f = mass * kd_point_accel(m, rc);
  n = mul(I, m.al) + cross(m.w, mul(I, m.w)) + cross(rc, f);
}

// Backward pass over a finger: with F, Nm = the wrench of links l .. 3 about o[l], joint l's torque -> t[l * ts] (registers, ts = 1,
// or the lane's LDS column, ts = KD_LD); the finger's wrench about o5 -> LDS words [WR, WR + 6): force, moment.
DI void kd_finger_backward(const V3* a, const V3* o, const V3* fl, const V3* nl, float* t, int ts, float* s_w, int WR, int lane) {
  V3 F = fl[3], Nm = nl[3];
  t[3 * ts] = dot(a[3], Nm);
#pragma unroll
  for (int l = DEXSIM_NFJ - 2; l >= 0; l--) {
    Nm = nl[l] + Nm + cross(o[l + 1] - o[l], F);
    F = fl[l] + F;
    t[l * ts] = dot(a[l], Nm);
  }
  Nm = Nm + cross(o[0], F);   // about o5
  KD_PUT3(WR, F);
  KD_PUT3(WR + 3, Nm);
}

// Palm pass: F, Nm = the palm link's wrench about o5; the five finger wrenches at LDS words [WR, WR + 30) are added and the sum is
// projected on the six base joints -> t[j * ts].  Links 0-4 are massless (validate_model): every base joint carries the whole hand.
DI void kd_palm_project(const KinBase& B, V3 F, V3 Nm, const float* s_w, int WR, int lane, float* t, int ts) {
#pragma unroll
  for (int ff = 0; ff < DEXSIM_NFINGER; ff++) {
    const float* const w = s_w + (WR + 6 * ff) * KD_LD + lane;
    F += v3(w[0], w[KD_LD], w[2 * KD_LD]);
    Nm += v3(w[3 * KD_LD], w[4 * KD_LD], w[5 * KD_LD]);
  }
#pragma unroll
  for (int j = 0; j < 6; j++)   // the moment about o_j: o5 - o_j = -orel[j]
    t[j * ts] = j < 3 ? dot(B.a[j], F) : dot(B.a[j], Nm - cross(B.orel[j], F));
}

// -------------------------------------------------------------------------------------------------- inverse dynamics
__global__ __launch_bounds__(KD_THREADS) void k_kin_invdyn(const DevParams* __restrict__ P, InvDyn K, int N, int NR) {
  __shared__ float s_w[ID_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;

  float qb[6], qf[4], vb[6], vf[4], ab[6], af[4];
  const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
  kd_load_qd(A, K.rows, K.qd, N, NR, f, vb, vf);
#pragma unroll
  for (int j = 0; j < 6; j++) ab[j] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++) af[j] = 0.f;
  if (K.qdd) kd_load_words(K.qdd, (size_t)kd_row(K.rows) * DEXSIM_NJ, 1, f, ab, af);
  KinBase B;
  kd_base_walk(P, qb, B);
  if (f == 0) s_valid[lane] = valid;

  // ---- forward pass: the base chain (every wave), then finger f; the link wrenches are formed on the way
  const V3 g = v3p(P->cfg.gravity);
  KdMotion mb[6];
  kd_base_motion(B, vb, ab, K.gravity ? v3(-g.x, -g.y, -g.z) : v3(0, 0, 0), mb);
  V3 a[4], o[4], fl[4], nl[4];
  {
    V3 of = v3(0, 0, 0), op = v3(0, 0, 0);
    Q4 qc = B.q[5];
    KdMotion m = mb[5];
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const JC& c = P->jc[6 + 4 * f + l];
      V3 rc;
      S6 I;
      kd_finger_link(c, qf[l], of, qc, a[l], rc, I);
      o[l] = of;
      m = kd_joint_motion(m, of - op, a[l], vf[l], af[l], false);
      op = of;
      kd_link_wrench(c.mass, rc, I, m, fl[l], nl[l]);
    }
  }
  // ---- backward and palm pass, spelled out: through kd_finger_backward and kd_palm_project tau on 65536 override rows was 4 % slower
  {
    V3 F = fl[3], Nm = nl[3];
    s_w[(ID_TAU + 6 + 4 * f + 3) * KD_LD + lane] = dot(a[3], Nm);
#pragma unroll
    for (int l = DEXSIM_NFJ - 2; l >= 0; l--) {
      Nm = nl[l] + Nm + cross(o[l + 1] - o[l], F);
      F = fl[l] + F;
      s_w[(ID_TAU + 6 + 4 * f + l) * KD_LD + lane] = dot(a[l], Nm);
    }
    Nm = Nm + cross(o[0], F);   // about o5
    KD_PUT3(ID_WR + 6 * f, F);
    KD_PUT3(ID_WR + 6 * f + 3, Nm);
  }
  __syncthreads();

  if (f == 0) {   // ---- palm pass: the palm link and the five fingers, projected on the six base joints
    V3 F, Nm;
    const JC& c5 = P->jc[5];
    const M3 R5 = q2mat(B.q[5]);
    kd_link_wrench(c5.mass, mul(R5, v3p(c5.com)), rotate_inertia(R5, c5.inertia), mb[5], F, Nm);
#pragma unroll
    for (int ff = 0; ff < DEXSIM_NFINGER; ff++) {
      const float* const w = s_w + (ID_WR + 6 * ff) * KD_LD + lane;
      F += v3(w[0], w[KD_LD], w[2 * KD_LD]);
      Nm += v3(w[3 * KD_LD], w[4 * KD_LD], w[5 * KD_LD]);
    }
#pragma unroll
    for (int j = 0; j < 6; j++)   // the moment about o_j: o5 - o_j = -orel[j]
      s_w[(ID_TAU + j) * KD_LD + lane] = j < 3 ? dot(B.a[j], F) : dot(B.a[j], Nm - cross(B.orel[j], F));
  }
  __syncthreads();
  kd_flush<false>(s_w, s_valid, ID_TAU, DEXSIM_NJ, K.tau);
}

// -------------------------------------------------------------------------------------------------- bias accelerations
// the bodies of the request that ride on joint frame j: a wave-uniform range of the sorted request
DI void ba_put_bodies(const DevParams* __restrict__ P, const BiasAcc& K, float* s_w, int lane, int j, const M3& Rj, const KdMotion& m) {
  for (int i = K.jstart[j + 1]; i < K.jstart[j + 2]; i++) {
    const int b = K.body[i], s = K.slot[i];
    const V3 lin = kd_point_accel(m, mul(Rj, v3p(P->model.body_p[b])));
    KD_PUT3(6 * s, lin); KD_PUT3(6 * s + 3, m.al);
  }
}

__global__ __launch_bounds__(KD_THREADS) void k_kin_bias_accel(const DevParams* __restrict__ P, BiasAcc K, int N, int NR) {
  __shared__ float s_w[BA_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;

  float qb[6], qf[4], vb[6], vf[4];
  const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
  kd_load_qd(A, K.rows, K.qd, N, NR, f, vb, vf);
  KinBase B;
  kd_base_walk(P, qb, B);
  KdMotion mb[6];
  kd_base_motion(B, vb, nullptr, v3(0, 0, 0), mb);
  if (f == 0) {
    s_valid[lane] = valid;
    for (int i = K.jstart[0]; i < K.jstart[1]; i++) {   // welded to the fixed spawn frame
      const int s = K.slot[i];
      KD_PUT3(6 * s, v3(0, 0, 0)); KD_PUT3(6 * s + 3, v3(0, 0, 0));
    }
#pragma unroll
    for (int j = 0; j < 6; j++) ba_put_bodies(P, K, s_w, lane, j, q2mat(B.q[j]), mb[j]);
  }
  V3 of = v3(0, 0, 0), op = v3(0, 0, 0);
  Q4 qc = B.q[5];
  KdMotion m = mb[5];
#pragma unroll
  for (int l = 0; l < DEXSIM_NFJ; l++) {
    const int j = 6 + 4 * f + l;
    V3 aw;
    kd_finger_joint(P->jc[j], qf[l], of, qc, aw);
    m = kd_joint_motion(m, of - op, aw, vf[l], 0.f, false);
    op = of;
    ba_put_bodies(P, K, s_w, lane, j, q2mat(qc), m);
  }
  __syncthreads();
  kd_flush<false>(s_w, s_valid, 0, 6 * K.nb, K.acc);
}
