// dexsim_fk.hip.inc -- forward kinematics of the hand (dexsim_forward_kinematics): the configuration the other queries describe --
// poses and twists of the published hand bodies (rows of rigid_body_states), poses of the DEXSIM_NSITE sites in the world or the hand
// frame, and the centroid record (centre of mass, its velocity, potential and kinetic energy) -- as functions of (q, qd).
//
// One kernel, not on the step path; it reads q and qd (arena rows or the caller's overrides) and writes caller-owned memory only, in
// the workgroup of dexsim_chain.hip.inc (64 rows x 5 waves, lanes along the rows, [word][row] LDS, o5-relative positions).  Every
// workgroup repeats the walk -- the base chain in every wave (kd_base_walk, kd_base_motion at qdd = 0), finger f in wave f -- and
// blockIdx.y says what it keeps of it:
//
//   y < nby   the bodies [FK_CHUNK y, FK_CHUNK (y + 1)) of the request, 13 words each as a rigid_body_states row has them; wave 0
//             stages the bodies welded to the spawn frame and the base frames, wave f those of its finger (kd_body_joint; the host
//             sorts every chunk by frame)
//   y == nby  the sites and the centroid: wave f stages sites 1 + f and 6 + f (wave 0 also site 0) and its finger's sums
//             (mass, m c, m v_c, kinetic energy; links 0..3 in order) about o5; after one __syncthreads() wave 0 adds the five
//             fingers in the order 0..4, then the palm link -- links 0-4 are massless (validate_model), exactly as k_kin_mass treats
//             them -- and shifts the centre by the world position of o5
//
// 37 x 13 words per row do not fit the static LDS, hence the chunks (as KJ_CHUNK); all of it is one launch.  The rows leave through
// kd_flush along the contiguous output index: word form for the bodies (13 nb is no multiple of 4) and the sites, quads for the centroid.
//
// From dexsim_chain.hip.inc: the row rule (kd_load_q, kd_load_qd), kd_base_walk, kd_finger_link, kd_flush; from dexsim_invdyn.hip.inc
// the angular part of the velocity walk (kd_base_motion, kd_joint_motion; their accelerations are dead code here).  The linear
// velocity of a frame's origin is carried next to it as publish_body does: v_j = v_parent + w_parent x (o_j - o_parent) [+ qd a].
//
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.
// Numerics: positions stay relative to o5 inside the walk; the world position of o5 (the spawn position, the walk's first increment,
// then its own suffix sum, as k_proximity forms it) is added once when a word is staged.  Without velocities (a q override without
// qd) every velocity word and the kinetic energy are stored as the constant +0.0f, not computed.

#define FK_CHUNK 19                                 /* bodies per workgroup (grid y): 37 bodies = 19 + 18 */
#define FK_BODY 13                                  /* words of a body: position, quaternion xyzw, linear, angular velocity */
#define FKS_SITE 0                                  /* [DEXSIM_NSITE][7] site poses, as they leave */
#define FKS_CEN (7 * DEXSIM_NSITE)                  /* [8] the centroid record, as it leaves */
#define FKS_PART (FKS_CEN + 8)                      /* [5][8] finger f's sums about o5: m, m c (3), m v_c (3), kinetic energy */
#define FKS_WORDS (FKS_PART + 8 * DEXSIM_NFINGER)
#define FK_WORDS (FK_CHUNK * FK_BODY > FKS_WORDS ? FK_CHUNK * FK_BODY : FKS_WORDS)
#define FK_MAX_CHUNKS ((DEXSIM_NUM_HAND_BODIES + FK_CHUNK - 1) / FK_CHUNK)
static_assert(FK_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_fk: static LDS above 64 KiB");

struct FwdKin {
  KinRows rows;
  const float* qd;         // (k, 26) override that goes with rows.q, or NULL
  float* body_states;      // (k, nb, 13) or NULL
  float* site_poses;       // (k, DEXSIM_NSITE, 7) or NULL
  float* centroid;         // (k, 8) or NULL
  int nb, nby;             // requested bodies, and the workgroups along y that carry them
  int vel;                 // the row has velocities: the state path, or an override with qd
  int hand_frame;          // DEXSIM_FK_HAND_FRAME
  // Each chunk of the request sorted by the frame a body rides on (host side), as BiasAcc has it, so that a wave visits its own
  // bodies only: entries [jstart[c][j + 1], jstart[c][j + 2]) of chunk c ride on joint frame j (j = -1: the fixed spawn frame); entry i
  // is body body[i], staged as body slot[i] of the chunk
  unsigned char body[DEXSIM_NUM_HAND_BODIES + 3], slot[DEXSIM_NUM_HAND_BODIES + 3];
  unsigned char jstart[FK_MAX_CHUNKS][DEXSIM_NJ + 2];
};

DI void fk_put_pose(float* s_w, int lane, int w, V3 p, Q4 q) {
  KD_PUT3(w, p);
  s_w[(w + 3) * KD_LD + lane] = q.x; s_w[(w + 4) * KD_LD + lane] = q.y; s_w[(w + 5) * KD_LD + lane] = q.z; s_w[(w + 6) * KD_LD + lane] = q.w;
}

// the bodies of chunk c that ride on joint frame j (-1: the spawn frame), a wave-uniform range of the sorted request: origin o
// relative to `base`, orientation qf, twist (vo at o, w) -- put_body of publish_body in these coordinates
DI void fk_put_bodies(const DevParams* __restrict__ P, const FwdKin& K, float* s_w, int lane, int c, int j, V3 base, V3 o, Q4 qf, V3 vo, V3 w) {
  const DexHandModel& M = P->model;
  const M3 R = q2mat(qf);
  for (int i = K.jstart[c][j + 1]; i < K.jstart[c][j + 2]; i++) {
    const int b = K.body[i], s = K.slot[i];
    const V3 r = mul(R, v3p(M.body_p[b]));
    const V3 v = vo + cross(w, r);
    fk_put_pose(s_w, lane, FK_BODY * s, base + (o + r), qmul(qf, q4p(M.body_q[b])));
    KD_PUT3(FK_BODY * s + 7, K.vel ? v : v3(0, 0, 0));
    KD_PUT3(FK_BODY * s + 10, K.vel ? w : v3(0, 0, 0));
  }
}

// a site welded to the frame (o relative to o5, qf): world pose, or the pose relative to site 0 (p0 relative to o5, q0) by the rule
// of the observation stage: p_h = qrot_inv(q_0, p - p_0), q_h = conj(q_0) (x) q
DI void fk_put_site(const DevParams* __restrict__ P, const FwdKin& K, float* s_w, int lane, int s, V3 o5w, V3 o, Q4 qf, const M3& R, V3 p0, Q4 q0) {
  const DexHandModel& M = P->model;
  const V3 p = o + mul(R, v3p(M.site_p[s]));
  const Q4 q = qmul(qf, q4p(M.site_q[s]));
  if (K.hand_frame) fk_put_pose(s_w, lane, FKS_SITE + 7 * s, qrot_inv(q0, p - p0), qmul(qconj(q0), q));
  else fk_put_pose(s_w, lane, FKS_SITE + 7 * s, o5w + p, q);
}

__global__ __launch_bounds__(KD_THREADS) void k_kin_fk(const DevParams* __restrict__ P, FwdKin K, int N, int NR) {
  __shared__ float s_w[FK_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const DexHandModel& M = P->model;

  float qb[6], qf[4], vb[6], vf[4];
  const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
#pragma unroll
  for (int j = 0; j < 6; j++) vb[j] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++) vf[j] = 0.f;
  if (K.vel) kd_load_qd(A, K.rows, K.qd, N, NR, f, vb, vf);
  if (f == 0) s_valid[lane] = valid;

  // ---- the base chain (every wave): frames, angular velocities, and the linear velocity of every origin
  KinBase B;
  kd_base_walk(P, qb, B);
  KdMotion mb[6];
  kd_base_motion(B, vb, nullptr, v3(0, 0, 0), mb);
  V3 vl[6];
  {
    V3 v = v3(0, 0, 0);
#pragma unroll
    for (int j = 0; j < 6; j++) {   // joint 0 hangs on a frame that does not turn: its lever never counts
      if (j > 0) v = v + cross(mb[j - 1].w, B.orel[j] - B.orel[j - 1]);
      if (j < 3) v += vb[j] * B.a[j];
      vl[j] = v;
    }
  }
  // o5 = spawn + (o_0 - spawn) + (o_5 - o_0): the first increment of the walk, then its own suffix sum
  const V3 inc0 = mul(q2mat(q4p(M.spawn_quat)), v3p(P->jc[0].poff)) + qb[0] * B.a[0];
  const V3 o5w = (v3p(M.spawn_pos) + inc0) - B.orel[0];

  if ((int)blockIdx.y < K.nby) {   // ---- a chunk of the requested bodies
    const int c = blockIdx.y, b0 = c * FK_CHUNK, nbc = min(FK_CHUNK, K.nb - b0);
    if (f == 0) {
      fk_put_bodies(P, K, s_w, lane, c, -1, v3(0, 0, 0), v3p(M.spawn_pos), q4p(M.spawn_quat), v3(0, 0, 0), v3(0, 0, 0));
#pragma unroll
      for (int j = 0; j < 6; j++) fk_put_bodies(P, K, s_w, lane, c, j, o5w, B.orel[j], B.q[j], vl[j], mb[j].w);
    }
    V3 of = v3(0, 0, 0), op = v3(0, 0, 0), v = vl[5];
    Q4 qc = B.q[5];
    KdMotion m = mb[5];
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const int j = 6 + 4 * f + l;
      V3 aw, rc;
      S6 I;
      kd_finger_link(P->jc[j], qf[l], of, qc, aw, rc, I);
      v = v + cross(m.w, of - op);
      m = kd_joint_motion(m, of - op, aw, vf[l], 0.f, false);
      op = of;
      fk_put_bodies(P, K, s_w, lane, c, j, o5w, of, qc, v, m.w);
    }
    __syncthreads();
    kd_flush<false, FK_CHUNK * FK_BODY>(s_w, s_valid, 0, FK_BODY * nbc, K.body_states, (size_t)FK_BODY * K.nb, (size_t)FK_BODY * b0);
    return;
  }

  // ---- the sites and the centroid
  const M3 R5 = q2mat(B.q[5]);
  const V3 p0 = mul(R5, v3p(M.site_p[0]));          // site 0 (right_hand_base) rides on joint 5 (validate_model)
  const Q4 q0 = qmul(B.q[5], q4p(M.site_q[0]));
  if (f == 0 && K.site_poses) fk_put_site(P, K, s_w, lane, 0, o5w, v3(0, 0, 0), B.q[5], R5, p0, q0);
  {
    V3 of = v3(0, 0, 0), op = v3(0, 0, 0), v = vl[5];
    Q4 qc = B.q[5];
    KdMotion m = mb[5];
    float sm = 0.f, ske = 0.f;
    V3 smc = v3(0, 0, 0), smv = v3(0, 0, 0);
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const JC& c = P->jc[6 + 4 * f + l];
      V3 aw, rc;
      S6 I;
      kd_finger_link(c, qf[l], of, qc, aw, rc, I);
      v = v + cross(m.w, of - op);
      m = kd_joint_motion(m, of - op, aw, vf[l], 0.f, false);
      op = of;
      if (K.centroid) {
        const V3 vc = v + cross(m.w, rc);
        sm += c.mass; smc += c.mass * (of + rc); smv += c.mass * vc;
        ske += 0.5f * (c.mass * dot(vc, vc) + dot(m.w, mul(I, m.w)));
      }
    }
    if (K.site_poses) {   // the tip and the pad of finger f ride on its last joint (validate_model)
      const M3 R = q2mat(qc);
      fk_put_site(P, K, s_w, lane, 1 + f, o5w, of, qc, R, p0, q0);
      fk_put_site(P, K, s_w, lane, 6 + f, o5w, of, qc, R, p0, q0);
    }
    if (K.centroid) {
      const int W = FKS_PART + 8 * f;
      s_w[W * KD_LD + lane] = sm;
      KD_PUT3(W + 1, smc); KD_PUT3(W + 4, smv);
      s_w[(W + 7) * KD_LD + lane] = ske;
    }
  }
  __syncthreads();
  if (K.centroid && f == 0) {   // fingers 0..4, then the palm link: one fixed order
    float sm = 0.f, ske = 0.f;
    V3 smc = v3(0, 0, 0), smv = v3(0, 0, 0);
#pragma unroll
    for (int ff = 0; ff < DEXSIM_NFINGER; ff++) {
      const float* const w = s_w + (FKS_PART + 8 * ff) * KD_LD + lane;
      sm += w[0];
      smc += v3(w[KD_LD], w[2 * KD_LD], w[3 * KD_LD]);
      smv += v3(w[4 * KD_LD], w[5 * KD_LD], w[6 * KD_LD]);
      ske += w[7 * KD_LD];
    }
    const JC& c5 = P->jc[5];
    const V3 rc = mul(R5, v3p(c5.com));
    const V3 vc = vl[5] + cross(mb[5].w, rc);
    const V3 w5 = mb[5].w;
    sm += c5.mass; smc += c5.mass * rc; smv += c5.mass * vc;
    ske += 0.5f * (c5.mass * dot(vc, vc) + dot(w5, mul(rotate_inertia(R5, c5.inertia), w5)));
    const float inv = 1.f / sm;   // the palm and the finger links have positive mass (validate_model)
    const V3 com = o5w + inv * smc;
    const V3 cv = inv * smv;
    const V3 g = v3p(P->cfg.gravity);
    KD_PUT3(FKS_CEN, com);
    s_w[(FKS_CEN + 3) * KD_LD + lane] = -(sm * dot(g, com));
    KD_PUT3(FKS_CEN + 4, K.vel ? cv : v3(0, 0, 0));
    s_w[(FKS_CEN + 7) * KD_LD + lane] = K.vel ? ske : 0.f;
  }
  __syncthreads();
  if (K.site_poses) kd_flush<false>(s_w, s_valid, FKS_SITE, 7 * DEXSIM_NSITE, K.site_poses);
  if (K.centroid) kd_flush<true>(s_w, s_valid, FKS_CEN, 8, K.centroid);
}
