// dexsim_chain.hip.inc -- the frame the query kernels share (k_render_scene, k_kin_jacobian, k_kin_mass, k_ik_solve, k_proximity,
// k_raycast, k_kin_fk, k_kin_invdyn, k_kin_bias_accel, k_kin_fwddyn, k_kin_id_deriv): pure functions of q (the last five of q and
// qd), off the step path, writing caller-owned memory only.  Force-inlined functions and macros only: this file emits no code of its
// own.
//
//   joint_frame      THE joint-frame rule: parent frame -> a joint's offset, world axis and frame.  Every walk of the family is
//                    written through it; publish_body (dexsim_physics.hip.inc) spells the same rule out for the step kernels.
//   kd_*             the workgroup shape of the tensor queries: 64 rows x 5 waves, lanes along the rows, wave f walks finger f
//                    (kd_base_walk, kd_finger_joint, kd_finger_link; sincos_joint, never jframe), positions RELATIVE TO THE PALM
//                    JOINT'S ORIGIN o5, per-row data staged in LDS as [word][row] with row stride KD_LD.
//   the row rule     kd_row / kd_env say which row and env a lane describes, kd_load_words reads its 6 + 4 words, kd_load puts the
//                    two together for an override or an arena field (kd_load_q, kd_load_qd).  A `valid` flag per row only gates
//                    stores: every lane reads legal addresses.  kd_flush writes rows that leave as they were staged, whole or as
//                    a range of columns of longer rows.
//   the scene stage  what the geometric queries (k_proximity, k_raycast) see of a row: KD_PLACE_HAND walks the hand and leaves the
//                    axis ends of the DEXSIM_NCAP collision capsules (capsule order: kd_finger_cap) and o5 (world) in LDS, running
//                    the kernel's ON_FRAME on every joint frame it stands on; KD_LOAD_BOX gives the row's box (KinBox) as a centre
//                    and a unit quaternion.
//   KD_TRI           the packed lower triangle every symmetric block of the family is kept in.

#define KD_LD 65          /* LDS row stride in words: [word][row], padded by one */
#define KD_THREADS 320    /* 5 waves: wave f walks finger f */

// A joint seen from its parent frame q_parent: d = R(q_parent) poff is the way from the parent's origin to the joint's (before
// a slide), aw the world axis R(qz) axis with qz = q_parent (x) qoff, qn the frame after the joint -- qz for a slide, which
// moves the origin by q aw, and qz (x) (axis sin(q / 2), cos(q / 2)) for a hinge.  The callers add d and the slide to their
// origin themselves: they associate that sum differently (world origins as (o + d) + q aw, the base walk as d + q aw).
struct JointFrame { V3 d, aw; Q4 qn; };

DI JointFrame joint_frame(const JC& c, float qj, Q4 q_parent, bool slide) {
  JointFrame F;
  F.d = mul(q2mat(q_parent), v3p(c.poff));
  const Q4 qz = qmul(q_parent, q4p(c.qoff));
  const V3 ax = v3p(c.axis);
  F.aw = mul(q2mat(qz), ax);
  F.qn = qz;
  if (!slide) { float s, cs; sincos_joint(0.5f * qj, &s, &cs); F.qn = qmul(qz, Q4{ax.x * s, ax.y * s, ax.z * s, cs}); }
  return F;
}

// ---- rows of a call: which env (or which override row) lane l describes
struct KinRows {
  const int64_t* env_ids;   // k ids or NULL = identity (state path only)
  const float* q;           // (k, 26) override or NULL = the arena's q of the row's env
  int k;
};

// hand body -> the joint frame it is welded to, as publish_body places them (-1 = the fixed spawn frame)
__host__ DI int kd_body_joint(int b) {
  if (b <= 6) return b == 6 ? 5 : b - 1;
  const int f = (b - 7) / 6, l = (b - 7) - 6 * f;
  return 6 + 4 * f + (l < 3 ? l : 3);
}

struct KinBase { V3 a[6], orel[6]; Q4 q[6]; };   // world axes, origins relative to o5, frame orientations of the base joints

// ---- the row rule: lane l = 64 blockIdx.x + lane describes row l of the call.  `valid` rows only decide about stores: every lane
// reads a legal address -- row min(l, k - 1) of a (k, ...) array, env 0 of the arena where the row has no env.
DI int kd_lane_row() { return blockIdx.x * 64 + (threadIdx.x & 63); }
DI int kd_row(const KinRows& R) { return min(kd_lane_row(), R.k - 1); }

// state path: the row's env (0 where it has none); `valid` also asks for an id inside [0, NR)
DI int kd_env(const KinRows& R, int NR, bool& valid) {
  long long id = kd_lane_row();
  if (R.env_ids) id = GPTR(R.env_ids)[kd_row(R)];
  valid = valid && id >= 0 && id < NR;
  return valid ? (int)id : 0;
}

// 6 base words + the 4 words of finger f out of 26, word j at p[at + j step]: row r of a (k, 26) array (at = 26 r, step = 1) or an
// arena field of env e (at = e, step = N)
DI void kd_load_words(const float* p, size_t at, size_t step, int f, float* b, float* w) {
#pragma unroll
  for (int j = 0; j < 6; j++) b[j] = GPTR(p)[at + j * step];
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = GPTR(p)[at + (6 + 4 * f + j) * step];
}

// the row's words of the (k, 26) override `ov`, else of the arena field `fld` of the row's env; returns `valid`
DI bool kd_load(const KinRows& R, const float* ov, const float* fld, int N, int NR, int f, float* b, float* w) {
  bool valid = kd_lane_row() < R.k;
  if (ov) kd_load_words(ov, (size_t)kd_row(R) * DEXSIM_NJ, 1, f, b, w);
  else kd_load_words(fld, kd_env(R, NR, valid), N, f, b, w);
  return valid;
}

// the row's q (6 base joints + the 4 joints of finger f) and, for the queries that are functions of (q, qd), its qd: `qd` is the
// (k, 26) override that goes with R.q (both NULL or both given), else the arena's qd of the env kd_load_q read q from
DI bool kd_load_q(const Arena& A, const KinRows& R, int N, int NR, int f, float* qb, float* qf) { return kd_load(R, R.q, A.q, N, NR, f, qb, qf); }
DI void kd_load_qd(const Arena& A, const KinRows& R, const float* qd, int N, int NR, int f, float* vb, float* vf) { kd_load(R, qd, A.qd, N, NR, f, vb, vf); }

DI void kd_base_walk(const DevParams* __restrict__ P, const float* qb, KinBase& B) {
  Q4 qc = q4p(P->model.spawn_quat);
  V3 inc[6];   // o_j - o_(j-1)
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const JointFrame F = joint_frame(P->jc[j], qb[j], qc, j < 3);
    V3 d = F.d;
    if (j < 3) d += qb[j] * F.aw;
    B.a[j] = F.aw; B.q[j] = F.qn; inc[j] = d; qc = F.qn;
  }
  B.orel[5] = v3(0, 0, 0);
#pragma unroll
  for (int j = 4; j >= 0; j--) B.orel[j] = B.orel[j + 1] - inc[j + 1];
}

// one joint of a finger chain: parent frame (of, qf) -> this joint's origin, world axis and frame
DI void kd_finger_joint(const JC& c, float qj, V3& of, Q4& qf, V3& aw) {
  const JointFrame F = joint_frame(c, qj, qf, false);
  of = of + F.d; aw = F.aw; qf = F.qn;
}

// one link of a finger chain: kd_finger_joint, then the link's centre (from the joint's origin) and inertia in world axes
DI void kd_finger_link(const JC& c, float qj, V3& of, Q4& qf, V3& aw, V3& rc, S6& I) {
  kd_finger_joint(c, qj, of, qf, aw);
  const M3 Rj = q2mat(qf);
  rc = mul(Rj, v3p(c.com));
  I = rotate_inertia(Rj, c.inertia);
}

#define KD_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))   /* packed lower triangle */
#define KD_PUT3(w, v) { s_w[((w) + 0) * KD_LD + lane] = (v).x; s_w[((w) + 1) * KD_LD + lane] = (v).y; s_w[((w) + 2) * KD_LD + lane] = (v).z; }

// ---- the scene stage of the geometric queries
// capsule of finger f's link l (cap_fslot == 3 f + l), behind the three palm capsules: the capsule order validate_model and
// dexsim_query_proximity insist on
__host__ DI int kd_finger_cap(int f, int l) { return 3 + 3 * f + l; }

// The box of a call (the host side is kin_box, dexsim_queries.hip); pose or env says that there is one
struct KinBox {
  const float* pose;   // (k, 7) centre xyz, quaternion xyzw, or NULL
  int env;             // no pose: the box of the row's env (state path, cfg.has_box)
  float hb;            // half edge of the box
};

// The two pieces below are macros, not functions, and stand in the kernel's own scope (P, A, M, K, N, NR, f, lane, s_w, s_valid, as
// KD_PUT3 does): the library is built with FMA contraction, which product of a sum of products is fused follows the order the
// optimiser hands the back end, and that order moved when these lines were reached through a call -- some of both kernels' words
// changed in their last bit.  As text in the kernel they compile to the instructions they compiled to when each kernel spelled them.
//
// KD_PLACE_HAND: lanes along the rows, wave f walks the chain of finger f (kd_load_q / kd_base_walk / kd_finger_joint) and leaves the
// axis ends p0.xyz p1.xyz of its three capsules, relative to o5, in the LDS words [cap0 + 6 c, cap0 + 6 c + 6); waves 0-2 also place
// one palm capsule each, wave 0 leaves o5 (world) in [o5w, o5w + 3) and the rows' `valid` in s_valid.  The wave that stands on a
// frame runs ON_WORLD(o) (wave 0, the env's world frame, o = -o5) or ON_FRAME(j, o, q) (wave 0 for the base joints 0..5, wave f for
// the joints 6 + 4 f + l of its finger; origin relative to o5, orientation), in front of the capsule that rides on j.  Sets `valid`;
// the caller's __syncthreads() publishes the words.
#define KD_PLACE_HAND(valid, cap0, o5w, ON_WORLD, ON_FRAME)                                                                   \
  {                                                                                                                           \
    float qb[6], qf[4];                                                                                                       \
    valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);                                                                           \
    KinBase B;                                                                                                                \
    kd_base_walk(P, qb, B);                                                                                                   \
    const M3 R5 = q2mat(B.q[5]);                                                                                              \
    if (f == 0) {                                                                                                             \
      s_valid[lane] = valid;                                                                                                  \
      /* o5 = spawn + (o_0 - spawn) + (o_5 - o_0): the first increment of the walk, then its own suffix sum */                \
      const V3 inc0 = mul(q2mat(q4p(M.spawn_quat)), v3p(P->jc[0].poff)) + qb[0] * B.a[0];                                     \
      const V3 o5 = (v3p(M.spawn_pos) + inc0) - B.orel[0];                                                                    \
      KD_PUT3(o5w, o5);                                                                                                       \
      ON_WORLD(v3(0, 0, 0) - o5);                                                                                             \
      _Pragma("unroll") for (int j = 0; j < 6; j++) ON_FRAME(j, B.orel[j], B.q[j]);                                           \
    }                                                                                                                         \
    if (f < 3) { /* palm capsule f rides on joint 5 (validate_model) */                                                       \
      const V3 p0 = mul(R5, v3p(M.cap_p0[f])), p1 = mul(R5, v3p(M.cap_p1[f]));                                                \
      KD_PUT3(cap0 + 6 * f, p0); KD_PUT3(cap0 + 6 * f + 3, p1);                                                               \
    }                                                                                                                         \
    V3 of = v3(0, 0, 0);                                                                                                      \
    Q4 qc = B.q[5];                                                                                                           \
    _Pragma("unroll") for (int l = 0; l < DEXSIM_NFJ; l++) {                                                                  \
      V3 aw;                                                                                                                  \
      kd_finger_joint(P->jc[6 + 4 * f + l], qf[l], of, qc, aw);                                                               \
      ON_FRAME(6 + 4 * f + l, of, qc);                                                                                        \
      if (l >= 1) { /* link l - 1 of the finger rides on its joint l (validate_model) */                                      \
        const int c = kd_finger_cap(f, l - 1);                                                                                \
        const M3 Rj = q2mat(qc);                                                                                              \
        const V3 p0 = of + mul(Rj, v3p(M.cap_p0[c])), p1 = of + mul(Rj, v3p(M.cap_p1[c]));                                    \
        KD_PUT3(cap0 + 6 * c, p0); KD_PUT3(cap0 + 6 * c + 3, p1);                                                             \
      }                                                                                                                       \
    }                                                                                                                         \
  }

// KD_LOAD_BOX: the box of row `row` (valid as KD_PLACE_HAND set it) into V3 bc and Q4 bq -- its row of K.box.pose, else, if ENV
// (K.box.env, or true where the caller stands under "the call has a box"), the arena fields of the row's env, else the identity
// at the origin.  The quaternion is normalised here (a zero quaternion is the identity): callers hand in rounded
// or integrated values.
#define KD_LOAD_BOX(bc, bq, row, valid, ENV)                                                                                  \
  V3 bc = v3(0, 0, 0);                                                                                                        \
  Q4 bq = {0.f, 0.f, 0.f, 1.f};                                                                                               \
  if (K.box.pose) {                                                                                                           \
    const float* const b = K.box.pose + (size_t)min((int)row, K.rows.k - 1) * 7;                                              \
    bc = v3(GPTR(b)[0], GPTR(b)[1], GPTR(b)[2]);                                                                              \
    bq = Q4{GPTR(b)[3], GPTR(b)[4], GPTR(b)[5], GPTR(b)[6]};                                                                  \
  } else if (ENV) {                                                                                                           \
    long long id = (long long)row;                                                                                            \
    if (K.rows.env_ids) id = GPTR(K.rows.env_ids)[min((int)row, K.rows.k - 1)];                                               \
    const int e = valid ? (int)id : 0;                                                                                        \
    bc = v3(FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2));                                                               \
    bq = Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)};                                          \
  }                                                                                                                           \
  {                                                                                                                           \
    const float n2 = bq.x * bq.x + bq.y * bq.y + bq.z * bq.z + bq.w * bq.w;                                                   \
    const bool ok = n2 > 1e-30f;                                                                                              \
    const float in = 1.f / sqrtf(ok ? n2 : 1.f);                                                                              \
    bq = Q4{ok ? bq.x * in : 0.f, ok ? bq.y * in : 0.f, ok ? bq.z * in : 0.f, ok ? bq.w * in : 1.f};                          \
  }

// Words [w0, w0 + n) of the workgroup's 64 staged rows -> dst[(row0 + r) * rowlen + col0 + c], all five waves along the contiguous
// output index; a row leaves only if s_valid[r].  QUAD: 16 bytes per lane (n a multiple of 4, dst 16-byte aligned), else one word.
// PER > 0: the index runs over PER >= n words per row, a compile-time constant, and the words past n are skipped.
template <bool QUAD, int PER = 0>
DI void kd_flush(const float* s_w, const int* s_valid, int w0, int n, float* dst, size_t rowlen, size_t col0) {
  const size_t row0 = (size_t)blockIdx.x * 64;
  const int per_row = PER ? PER : QUAD ? n / 4 : n;
  for (int idx = threadIdx.x; idx < 64 * per_row; idx += KD_THREADS) {
    const int r = idx / per_row, c = idx - r * per_row;
    if ((PER && c >= n) || !s_valid[r]) continue;
    if (QUAD) {
      const float* const w = s_w + (w0 + 4 * c) * KD_LD + r;
      st4_global(dst + (row0 + r) * rowlen + col0 + 4 * (size_t)c, w[0], w[KD_LD], w[2 * KD_LD], w[3 * KD_LD]);
    } else {
      GPTR(dst)[(row0 + r) * rowlen + col0 + c] = s_w[(w0 + c) * KD_LD + r];
    }
  }
}

// rows of n words that leave whole
template <bool QUAD>
DI void kd_flush(const float* s_w, const int* s_valid, int w0, int n, float* dst) { kd_flush<QUAD>(s_w, s_valid, w0, n, dst, n, 0); }
