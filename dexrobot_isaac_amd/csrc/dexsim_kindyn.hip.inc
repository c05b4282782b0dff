// dexsim_kindyn.hip.inc -- kinematics / dynamics tensors of the hand (dexsim_body_jacobian, dexsim_mass_matrix): the geometric
// Jacobians of the published hand bodies, the joint-space inertia M(q) and the gravity force dV/dq, all pure functions of q.
//
// Two kernels, neither on the step path; both read q (arena rows or the caller's override) and write caller-owned memory only.
// The outputs are large AoS rows (up to 37 x 156 words of Jacobian, 676 words of M per row), so each kernel works in two phases
// inside the workgroup of dexsim_chain.hip.inc (64 rows x 5 waves, [word][row] LDS, o5-relative positions):
//
//   phase A  lanes along the rows; wave f walks the chain of finger f (kd_base_walk, kd_finger_joint) and leaves the COMPACT
//            per-row data in LDS (a phase-A write is 64 consecutive banks, a phase-B read of many words of one row is too):
//              k_kin_jacobian  26 world axes, 26 joint origins, the origins of the <= KJ_CHUNK bodies of this workgroup's chunk
//              k_kin_mass      the 191 unique words of M (21 base + 5 x (10 finger + 24 base-finger)) and 26 gravity words
//   phase B  all 5 waves along the CONTIGUOUS output index: expand to the dense layout -- cross product a_c x (p_b - o_c) or
//            a_c, ancestor mask, symmetric mirror, exact zeros -- and store 16 bytes per lane, fully coalesced.
//
// From dexsim_chain.hip.inc: the row rule (kd_load_q), kd_base_walk, kd_finger_joint (Jacobians) and the link walk kd_finger_link
// (mass matrix), KD_TRI, kd_flush.  kd_base_block, defined here, is also k_kin_fwddyn's (dexsim_fwddyn.hip.inc).
//
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.
//
// Numerics: with positions relative to o5 (the finger walk starts at 0, the base origins are suffix sums of the walk's own
// increments) levers and composite centres are differences of numbers of hand size (< 0.4 m),
// not of world coordinates; the composites of the CRBA are formed about their own centres of mass in these coordinates.  The
// spawn position therefore never enters.  Link inertias are general symmetric tensors (rotate_inertia), not DevParams::inertia_diag.

// -------------------------------------------------------------------------------------------------- body Jacobians
#define KJ_CHUNK 10                      /* bodies per workgroup (grid y): 37 bodies = 10 + 10 + 10 + 7 */
#define KJ_AX 0                          /* [26][3] world axes */
#define KJ_OR (3 * DEXSIM_NJ)            /* [26][3] joint origins relative to o5 */
#define KJ_BP (6 * DEXSIM_NJ)            /* [KJ_CHUNK][3] body origins relative to o5 */
#define KJ_WORDS (KJ_BP + 3 * KJ_CHUNK)
#define KJ_ROW (6 * DEXSIM_NJ)           /* words of one body's Jacobian */
static_assert(KJ_ROW % 4 == 0, "a body's Jacobian is written as 16-byte quads");
static_assert(KJ_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_jacobian: static LDS above 64 KiB");

struct KinJac {
  KinRows rows;
  float* jac;                                  // (k, nb, 6, 26)
  int nb;
  unsigned char body[DEXSIM_NUM_HAND_BODIES + 3];   // the nb requested bodies
};

__global__ __launch_bounds__(KD_THREADS) void k_kin_jacobian(const DevParams* __restrict__ P, KinJac J, int N, int NR) {
  __shared__ float s_w[KJ_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const DexHandModel& M = P->model;
  const int b0 = blockIdx.y * KJ_CHUNK, nbc = min(KJ_CHUNK, J.nb - b0);

  {   // ---- phase A
    float qb[6], qf[4];
    const bool valid = kd_load_q(A, J.rows, N, NR, f, qb, qf);
    KinBase B;
    kd_base_walk(P, qb, B);
    if (f == 0) {
      s_valid[lane] = valid;
#pragma unroll
      for (int j = 0; j < 6; j++) { KD_PUT3(KJ_AX + 3 * j, B.a[j]); KD_PUT3(KJ_OR + 3 * j, B.orel[j]); }
      for (int s = 0; s < nbc; s++) {   // bodies of the chunk that ride on the base chain (wave-uniform branches)
        const int b = J.body[b0 + s], pj = kd_body_joint(b);
        if (pj < 0) { KD_PUT3(KJ_BP + 3 * s, v3(0, 0, 0)); }
#pragma unroll
        for (int j = 0; j < 6; j++)
          if (pj == j) { const V3 p = B.orel[j] + mul(q2mat(B.q[j]), v3p(M.body_p[b])); KD_PUT3(KJ_BP + 3 * s, p); }
      }
    }
    V3 of = v3(0, 0, 0);
    Q4 qc = B.q[5];
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const int j = 6 + 4 * f + l;
      V3 aw;
      kd_finger_joint(P->jc[j], qf[l], of, qc, aw);
      KD_PUT3(KJ_AX + 3 * j, aw); KD_PUT3(KJ_OR + 3 * j, of);
      const M3 Rj = q2mat(qc);
      for (int s = 0; s < nbc; s++) {
        const int b = J.body[b0 + s];
        if (kd_body_joint(b) == j) { const V3 p = of + mul(Rj, v3p(M.body_p[b])); KD_PUT3(KJ_BP + 3 * s, p); }
      }
    }
  }
  __syncthreads();

  // ---- phase B: quad t of row r is words [4 t, 4 t + 4) of the chunk's nbc x 156 contiguous words of that row
  const int per_row = nbc * (KJ_ROW / 4);
  const size_t row0 = (size_t)blockIdx.x * 64;
  for (int idx = threadIdx.x; idx < 64 * per_row; idx += KD_THREADS) {
    const int r = idx / per_row, t = idx - r * per_row;
    if (!s_valid[r]) continue;
    const int s = t / (KJ_ROW / 4), u = t - s * (KJ_ROW / 4);
    const int pj = kd_body_joint(J.body[b0 + s]);
    const float* const w = s_w + r;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int el = 4 * u + i, d = el / DEXSIM_NJ, c = el - d * DEXSIM_NJ;
      const bool anc = c <= pj && (c < 6 || ((c - 6) >> 2) == ((pj - 6) >> 2));   // joint c moves the body
      const int d0 = d < 3 ? d : d - 3, d1 = d0 == 2 ? 0 : d0 + 1, d2 = d0 == 0 ? 2 : d0 - 1;
      const float a0 = w[(KJ_AX + 3 * c + d0) * KD_LD], a1 = w[(KJ_AX + 3 * c + d1) * KD_LD], a2 = w[(KJ_AX + 3 * c + d2) * KD_LD];
      const float r1 = w[(KJ_BP + 3 * s + d1) * KD_LD] - w[(KJ_OR + 3 * c + d1) * KD_LD];
      const float r2 = w[(KJ_BP + 3 * s + d2) * KD_LD] - w[(KJ_OR + 3 * c + d2) * KD_LD];
      const float lin = c < 3 ? a0 : a1 * r2 - a2 * r1;   // a_c, or (a_c x (p_b - o_c))[d0]
      const float ang = c < 3 ? 0.f : a0;
      v[i] = anc ? (d < 3 ? lin : ang) : 0.f;
    }
    st4_global(J.jac + ((row0 + r) * J.nb + b0) * KJ_ROW + 4 * (size_t)t, v[0], v[1], v[2], v[3]);
  }
}

// -------------------------------------------------------------------------------------------------- mass matrix and gravity force
// LDS words: the gravity force of joint j at KM_GRAV + j, as it leaves.  Per finger f at KM_FINGER(f): [0, 10) lower triangle of
// the finger's 4 x 4 block (row l, column l2 <= l at l (l + 1) / 2 + l2), [10, 34) coupling of finger joint l with base joint k at
// 10 + 6 l + k.  The base pass (wave 0) reads the five finger composites from KM_BASE + [0, 50) and then writes the 21 words of
// its own block over them: that column of the region belongs to its lane alone.
#define KM_GRAV 0                              /* [26] gravity force */
#define KM_FWORDS 34
#define KM_FINGER(f) (DEXSIM_NJ + (f) * KM_FWORDS)
#define KM_BASE KM_FINGER(DEXSIM_NFINGER)      /* [0, 21) lower triangle of the base block */
#define KM_COMP_WORDS 10                       /* m, c (3), I (6) of a finger's composite */
#define KM_WORDS (KM_BASE + DEXSIM_NFINGER * KM_COMP_WORDS)
#define KM_ROW (DEXSIM_NJ * DEXSIM_NJ)
static_assert(KM_ROW % 4 == 0, "M is written as 16-byte quads");
static_assert(KM_WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_mass: static LDS above 64 KiB");

struct KinMass {
  KinRows rows;
  float* mass;      // (k, 26, 26) or NULL
  float* gravity;   // (k, 26) or NULL
};

// M[i][j] of row r from the compact words (both triangles from the one word; finger-finger cross blocks are exact zeros)
DI float kd_mass_entry(const float* s_w, int r, int i, int j) {
  const int hi = max(i, j), lo = min(i, j);
  int w;
  bool zero = false;
  if (hi < 6) w = KM_BASE + KD_TRI(hi, lo);
  else {
    const int f = (hi - 6) >> 2, l = (hi - 6) & 3;
    if (lo < 6) w = KM_FINGER(f) + 10 + 6 * l + lo;
    else { const int l2 = (lo - 6) & 3; zero = ((lo - 6) >> 2) != f; w = KM_FINGER(f) + KD_TRI(l, l2); }
  }
  const float v = s_w[w * KD_LD + r];
  return zero ? 0.f : v;
}

// The composite-body words (CRBA).  For the subtree of joint i with composite H (mass, centre relative to o5, inertia about the
// centre) and axis a_i: Pm = m dc/dq_i is its momentum for unit velocity, L = I a_i its angular momentum about the centre, and
// M[i][k], k an ancestor of i (or i), is a_k . Pm (k prismatic) or a_k . (L + (c - o_k) x Pm) (k revolute); dV/dq_i = -g . Pm.

// the 21 words a rigid body H adds to the base block: every base joint carries it -> out[KD_TRI(i, k)]
DI void kd_base_block(const KinBase& B, const Comp& H, float* out) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const V3 Pm = H.m * (i < 3 ? B.a[i] : cross(B.a[i], H.c - B.orel[i]));
    const V3 L = i < 3 ? v3(0, 0, 0) : mul(H.I, B.a[i]);
#pragma unroll
    for (int k = 0; k <= i; k++) out[KD_TRI(i, k)] = k < 3 ? dot(B.a[k], Pm) : dot(B.a[k], L + cross(H.c - B.orel[k], Pm));
  }
}

__global__ __launch_bounds__(KD_THREADS) void k_kin_mass(const DevParams* __restrict__ P, KinMass K, int N, int NR) {
  __shared__ float s_w[KM_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const V3 g = v3p(P->cfg.gravity);

  {   // ---- phase A, finger pass: every wave its finger
    float qb[6], qf[4];
    const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
    KinBase B;
    kd_base_walk(P, qb, B);
    if (f == 0) s_valid[lane] = valid;
    V3 a[4], o[4];
    Comp comp[4];
    {
      V3 of = v3(0, 0, 0);
      Q4 qc = B.q[5];
#pragma unroll
      for (int l = 0; l < DEXSIM_NFJ; l++) {
        const JC& c = P->jc[6 + 4 * f + l];
        V3 rc;
        kd_finger_link(c, qf[l], of, qc, a[l], rc, comp[l].I);
        o[l] = of;
        comp[l].m = c.mass; comp[l].c = of + rc;
      }
    }
#pragma unroll
    for (int l = DEXSIM_NFJ - 2; l >= 0; l--) comp_add(comp[l], comp[l + 1]);   // subtree of joint l = links l .. 3
    const int F = KM_FINGER(f);
#pragma unroll
    for (int i = 0; i < DEXSIM_NFJ; i++) {   // spelled out here and in k_kin_fwddyn: through one kd_finger_blocks the mass solve rounded differently
      const V3 Pm = comp[i].m * cross(a[i], comp[i].c - o[i]);
      const V3 L = mul(comp[i].I, a[i]);
#pragma unroll
      for (int k = 0; k <= i; k++) s_w[(F + KD_TRI(i, k)) * KD_LD + lane] = dot(a[k], L + cross(comp[i].c - o[k], Pm));
#pragma unroll
      for (int k = 0; k < 6; k++)
        s_w[(F + 10 + 6 * i + k) * KD_LD + lane] = k < 3 ? dot(B.a[k], Pm) : dot(B.a[k], L + cross(comp[i].c - B.orel[k], Pm));
      s_w[(KM_GRAV + 6 + 4 * f + i) * KD_LD + lane] = -dot(g, Pm);
    }
    {   // the finger's composite for the base pass
      const int W = KM_BASE + KM_COMP_WORDS * f;
      const Comp& c = comp[0];
      s_w[W * KD_LD + lane] = c.m;
      KD_PUT3(W + 1, c.c);
      s_w[(W + 4) * KD_LD + lane] = c.I.xx; s_w[(W + 5) * KD_LD + lane] = c.I.yy; s_w[(W + 6) * KD_LD + lane] = c.I.zz;
      s_w[(W + 7) * KD_LD + lane] = c.I.xy; s_w[(W + 8) * KD_LD + lane] = c.I.xz; s_w[(W + 9) * KD_LD + lane] = c.I.yz;
    }
    __syncthreads();

    if (f == 0) {   // ---- phase A, base pass: links 0-4 are massless (validate_model), so every base joint carries the whole hand
      const JC& c5 = P->jc[5];
      const M3 R5 = q2mat(B.q[5]);
      Comp H;
      H.m = c5.mass; H.c = mul(R5, v3p(c5.com)); H.I = rotate_inertia(R5, c5.inertia);
#pragma unroll
      for (int ff = 0; ff < DEXSIM_NFINGER; ff++) {
        const float* const w = s_w + (KM_BASE + KM_COMP_WORDS * ff) * KD_LD + lane;
        Comp c;
        c.m = w[0]; c.c = v3(w[KD_LD], w[2 * KD_LD], w[3 * KD_LD]);
        c.I = S6{w[4 * KD_LD], w[5 * KD_LD], w[6 * KD_LD], w[7 * KD_LD], w[8 * KD_LD], w[9 * KD_LD]};
        comp_add(H, c);
      }
      float out[21], grav[6];   // spelled out: through kd_base_block, M[5][4] and M[5][5] rounded differently
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const V3 Pm = H.m * (i < 3 ? B.a[i] : cross(B.a[i], H.c - B.orel[i]));
        const V3 L = i < 3 ? v3(0, 0, 0) : mul(H.I, B.a[i]);
#pragma unroll
        for (int k = 0; k <= i; k++) out[KD_TRI(i, k)] = k < 3 ? dot(B.a[k], Pm) : dot(B.a[k], L + cross(H.c - B.orel[k], Pm));
        grav[i] = -dot(g, Pm);
      }
#pragma unroll
      for (int i = 0; i < 21; i++) s_w[(KM_BASE + i) * KD_LD + lane] = out[i];   // over the composites: all of them are in registers
#pragma unroll
      for (int i = 0; i < 6; i++) s_w[(KM_GRAV + i) * KD_LD + lane] = grav[i];
    }
  }
  __syncthreads();

  // ---- phase B
  const size_t row0 = (size_t)blockIdx.x * 64;
  if (K.mass) {
    for (int idx = threadIdx.x; idx < 64 * (KM_ROW / 4); idx += KD_THREADS) {
      const int r = idx / (KM_ROW / 4), u = idx - r * (KM_ROW / 4);
      if (!s_valid[r]) continue;
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int t = 4 * u + i, ii = t / DEXSIM_NJ, jj = t - ii * DEXSIM_NJ;
        v[i] = kd_mass_entry(s_w, r, ii, jj);
      }
      st4_global(K.mass + (row0 + r) * KM_ROW + 4 * (size_t)u, v[0], v[1], v[2], v[3]);
    }
  }
  if (K.gravity) kd_flush<false>(s_w, s_valid, KM_GRAV, DEXSIM_NJ, K.gravity);
}
