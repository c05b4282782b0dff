// dexsim_chain.hip.inc -- the frame the query kernels share (k_render_scene, k_kin_jacobian, k_kin_mass, k_ik_solve, k_proximity,
// k_kin_invdyn, k_kin_bias_accel): pure functions of q (the last two of q and qd: kd_load_qd), off the step path, writing
// caller-owned memory only.  Force-inlined functions and macros only: this file emits no code of its own.
//
//   joint_frame      THE joint-frame rule: parent frame -> a joint's offset, world axis and frame.  Every walk of the family is
//                    written through it; publish_body (dexsim_physics.hip.inc) spells the same rule out for the step kernels.
//   kd_*             the workgroup shape of the tensor queries: 64 rows x 5 waves, lanes along the rows, wave f walks finger f
//                    (kd_load_q, kd_base_walk, kd_finger_joint; sincos_joint, never jframe), positions RELATIVE TO THE PALM
//                    JOINT'S ORIGIN o5, per-row data staged in LDS as [word][row] with row stride KD_LD, a `valid` flag per row
//                    that only gates stores (every lane reads legal addresses), kd_flush for rows that leave as they were staged.

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

// the row's q: 6 base joints + the 4 joints of finger f.  `valid` rows only decide about stores: every lane reads a legal address
DI bool kd_load_q(const Arena& A, const KinRows& R, int N, int NR, int f, float* qb, float* qf) {
  const int l = blockIdx.x * 64 + (threadIdx.x & 63);
  bool valid = l < R.k;
  if (R.q) {
    const size_t row = (size_t)min(l, R.k - 1) * DEXSIM_NJ;
#pragma unroll
    for (int j = 0; j < 6; j++) qb[j] = GPTR(R.q)[row + j];
#pragma unroll
    for (int j = 0; j < 4; j++) qf[j] = GPTR(R.q)[row + 6 + 4 * f + j];
  } else {
    long long id = l;
    if (R.env_ids) id = GPTR(R.env_ids)[min(l, R.k - 1)];
    valid = valid && id >= 0 && id < NR;
    const int e = valid ? (int)id : 0;
#pragma unroll
    for (int j = 0; j < 6; j++) qb[j] = FLD(q, j);
#pragma unroll
    for (int j = 0; j < 4; j++) qf[j] = FLD(q, 6 + 4 * f + j);
  }
  return valid;
}

// the row's qd, for the queries that are functions of (q, qd): `qd` is the (k, 26) override that goes with R.q (both NULL or both
// given), else the arena's qd of the env kd_load_q read q from.  Like kd_load_q, every lane reads a legal address.
DI void kd_load_qd(const Arena& A, const KinRows& R, const float* qd, int N, int NR, int f, float* vb, float* vf) {
  const int l = blockIdx.x * 64 + (threadIdx.x & 63);
  if (qd) {
    const size_t row = (size_t)min(l, R.k - 1) * DEXSIM_NJ;
#pragma unroll
    for (int j = 0; j < 6; j++) vb[j] = GPTR(qd)[row + j];
#pragma unroll
    for (int j = 0; j < 4; j++) vf[j] = GPTR(qd)[row + 6 + 4 * f + j];
  } else {
    long long id = l;
    if (R.env_ids) id = GPTR(R.env_ids)[min(l, R.k - 1)];
    const int e = (l < R.k && id >= 0 && id < NR) ? (int)id : 0;
#pragma unroll
    for (int j = 0; j < 6; j++) vb[j] = FLD(qd, j);
#pragma unroll
    for (int j = 0; j < 4; j++) vf[j] = FLD(qd, 6 + 4 * f + j);
  }
}

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

#define KD_PUT3(w, v) { s_w[((w) + 0) * KD_LD + lane] = (v).x; s_w[((w) + 1) * KD_LD + lane] = (v).y; s_w[((w) + 2) * KD_LD + lane] = (v).z; }

// Words [w0, w0 + n) of the workgroup's 64 staged rows -> dst[(row0 + r) * n + c], all five waves along the contiguous output
// index; a row leaves only if s_valid[r].  QUAD: 16 bytes per lane (n a multiple of 4, dst 16-byte aligned), else one word.
template <bool QUAD>
DI void kd_flush(const float* s_w, const int* s_valid, int w0, int n, float* dst) {
  const size_t row0 = (size_t)blockIdx.x * 64;
  const int per_row = QUAD ? n / 4 : n;
  for (int idx = threadIdx.x; idx < 64 * per_row; idx += KD_THREADS) {
    const int r = idx / per_row, c = idx - r * per_row;
    if (!s_valid[r]) continue;
    if (QUAD) {
      const float* const w = s_w + (w0 + 4 * c) * KD_LD + r;
      st4_global(dst + (row0 + r) * n + 4 * (size_t)c, w[0], w[KD_LD], w[2 * KD_LD], w[3 * KD_LD]);
    } else {
      GPTR(dst)[(row0 + r) * n + c] = s_w[(w0 + c) * KD_LD + r];
    }
  }
}
