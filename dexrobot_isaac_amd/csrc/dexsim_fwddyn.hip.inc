// dexsim_fwddyn.hip.inc -- forward dynamics and mass-matrix solves of the hand (dexsim_forward_dynamics, dexsim_mass_solve):
// qdd = (M(q) [+ A])^-1 (tau - c(q, qd) [- g(q)]) and out = (M(q) [+ A])^-1 rhs for up to DEXSIM_MSOLVE_MAX_RHS right-hand sides, with
// the M, c and g of dexsim_mass_matrix / dexsim_inverse_dynamics and A = diag(DexHandModel::armature).  M is never written out.
//
// One kernel template, off the step path, in the workgroup of dexsim_chain.hip.inc (64 rows x 5 waves, lanes along the rows,
// [word][row] LDS, o5-relative positions).  M is block-arrow -- a 6 x 6 base block B, five 4 x 4 finger blocks F_f, five 6 x 4
// couplings C_f, exact zeros between fingers -- and is solved as the sub-step solves its own matrix (dexsim_physics.hip.inc):
// eliminate the fingers, Cholesky of the 6 x 6 Schur complement on wave 0, back-substitute.  NOT the articulated-body recursion:
// projecting a 6 x 6 articulated inertia five times through the massless base joints cancels in fp32.
//
//   setup   every wave repeats the base chain and walks finger f.  FD: the Newton-Euler pass of k_kin_invdyn at
//           qdd = 0 gives the bias force (kd_joint_motion, kd_link_wrench on the rotated centre and inertia the composites share,
//           kd_finger_backward: the finger's joints stay in registers, its wrench about o5 goes to LDS for kd_palm_project).
//           Both: the composite-body words F_f, C_f (k_kin_mass's loop, spelled out again: see there), F_f (+ A) inverted
//           (spd_inverse<4>), G_f = F_f^-1 C_f^T.
//           B is a sum over bodies, so the finger's own composite gives its part B_f of B on its own wave, and what goes to LDS is
//           the finger's 21 words of the Schur complement, B_f - C_f F_f^-1 C_f^T: wave 0 is left with the palm link alone.
//   factor  wave 0, after the first barrier: S = B_palm (+ A) + the five finger parts, fd_chol6 -- once per row
//   columns per batch of CB right-hand sides (FD: its one):  all waves stage the rows' words through LDS along the contiguous index
//           | fingers: y_f = F_f^-1 r_f in place, C_f F_f^-1 r_f = G_f^T r_f -> LDS | wave 0: x_B = S^-1 (r_B - sum_f G_f^T r_f) in
//           place | fingers: x_f = y_f - G_f x_B in place | all waves flush.  One __syncthreads() between the stages.
//
// FD is the instance with one column whose right-hand side is tau - bias; everything after that subtraction is the code of the
// mass solve, so at qd = 0 without gravity (the Newton-Euler pass gives exact zeros) the two return the same bits.  A column's
// arithmetic does not depend on the batch it sits in.  In place (out == rhs) is safe: a batch is read before it is written and
// no other batch or workgroup touches its words.
//
// From dexsim_chain.hip.inc: the row rule (kd_load_q, kd_load_qd), kd_base_walk, kd_finger_joint, KD_TRI, kd_flush (whole
// rows for FD, a batch of columns inside rows of nrhs x 26 words for the mass solve).  From dexsim_invdyn.hip.inc: the Newton-Euler
// set.  From dexsim_kindyn.hip.inc: kd_base_block.
//
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.

#ifndef FD_COLS
#define FD_COLS 4        /* right-hand sides per barrier round of the mass solve (1 .. 4; profiles/forward_dynamics/README.md) */
#endif
static_assert(FD_COLS >= 1 && FD_COLS <= 4, "FD_COLS: the batch has to fit the 64 KiB of static LDS");

// LDS words.  SCH is dead once wave 0 has its factor, so the mass solve (one barrier more per launch) puts CFR over it.
template <bool FD>
struct FdMap {
  static constexpr int CB = FD ? 1 : FD_COLS;                          // columns per batch
  static constexpr int SCH = 0;                                        // [5][21] finger f's part of the Schur complement
  static constexpr int WR = 21 * DEXSIM_NFINGER;                       // [5][6] FD: finger f's wrench about o5
  static constexpr int M5 = WR + 6 * DEXSIM_NFINGER;                   // [9] FD: motion of the palm frame (w, al, ao), wave 0's own
  static constexpr int CFR = FD ? M5 + 9 : 0;                          // [CB][5][6] G_f^T r_f
  static constexpr int CFR_END = CFR + CB * 6 * DEXSIM_NFINGER;
  static constexpr int STAGE = CFR_END > WR ? CFR_END : WR;            // [CB][26] the columns, in place from rhs to result
  static constexpr int WORDS = STAGE + CB * DEXSIM_NJ;
};
static_assert(FdMap<true>::WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_fwddyn<true>: static LDS above 64 KiB");
static_assert(FdMap<false>::WORDS * KD_LD * 4 + 256 <= 65536, "k_kin_fwddyn<false>: static LDS above 64 KiB");

struct FwdDyn {
  KinRows rows;
  const float* qd;     // FD: (k, 26) override that goes with rows.q, or NULL = the arena's qd
  const float* rhs;    // (k, nrhs, 26) aligned with the output rows; FD: tau (nrhs = 1), NULL = zero
  float* out;          // (k, nrhs, 26); may be rhs
  int nrhs;
  int gravity;         // FD: DEXSIM_FD_GRAVITY
  int armature;        // DEXSIM_FD_ARMATURE
};

// Where a value of the code both instances share is also read by the Newton-Euler pass of FD, it goes through opaque() in BOTH:
// the compiler contracts a product into a following add only if the product has no other reader, so a second reader in one
// instance would change the rounding of the shared arithmetic, and forward dynamics at qd = 0 would lose the bits of the mass solve.
DI V3 fd_opaque(V3 v) { return {opaque(v.x), opaque(v.y), opaque(v.z)}; }
DI S6 fd_opaque(S6 s) { return {opaque(s.xx), opaque(s.yy), opaque(s.zz), opaque(s.xy), opaque(s.xz), opaque(s.yz)}; }

// Cholesky factor of a packed SPD 6 x 6 (spd_solve<6>'s arithmetic, the factor kept): L below the diagonal, rd = 1 / L_ii
DI void fd_chol6(const float* S, float* L, float* rd) {
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = S[KD_TRI(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s -= L[KD_TRI(i, k)] * L[KD_TRI(j, k)];
      if (i == j) { const float d = sqrtf(fmaxf(s, 1e-20f)); L[KD_TRI(i, i)] = d; rd[i] = 1.f / d; }
      else L[KD_TRI(i, j)] = s * rd[j];
    }
}

DI void fd_chol6_solve(const float* L, const float* rd, const float* b, float* x) {
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= L[KD_TRI(i, k)] * y[k];
    y[i] = s * rd[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    float s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s -= L[KD_TRI(k, i)] * x[k];
    x[i] = s * rd[i];
  }
}

// Columns [c0, c0 + CB) of the workgroup's 64 rows, global -> registers -> LDS, all five waves along the contiguous index: word c
// of row r's CW = 26 CB contiguous words (fewer in the last batch) belongs to thread (r CW + c) mod 320, round (r CW + c) / 320.
// Load and LDS write are two calls, so that the loads of a batch are in flight while other work runs.  Every lane reads a legal
// address (a word outside the batch reads the batch's last one and is never used).
template <int CW, int TIN>
DI void fd_cols_load(const FwdDyn& K, int c0, float* tin) {
  const int n = min(CW, (K.nrhs - c0) * DEXSIM_NJ);
  const size_t rowlen = (size_t)K.nrhs * DEXSIM_NJ;
#pragma unroll
  for (int i = 0; i < TIN; i++) {
    const int idx = threadIdx.x + i * KD_THREADS, r = min(idx / CW, 63), c = min(idx - (idx / CW) * CW, n - 1);
    const size_t row = (size_t)min((int)blockIdx.x * 64 + r, K.rows.k - 1);
    tin[i] = K.rhs ? GPTR(K.rhs)[row * rowlen + (size_t)c0 * DEXSIM_NJ + c] : 0.f;
  }
}

template <int CW, int TIN>
DI void fd_cols_stage(float* s_w, int w0, const float* tin) {
#pragma unroll
  for (int i = 0; i < TIN; i++) {
    const int idx = threadIdx.x + i * KD_THREADS, r = idx / CW, c = idx - r * CW;
    if (idx < 64 * CW) s_w[(w0 + c) * KD_LD + r] = tin[i];
  }
}

template <bool FD>
__global__ __launch_bounds__(KD_THREADS) void k_kin_fwddyn(const DevParams* __restrict__ P, FwdDyn K, int N, int NR) {
  using Map = FdMap<FD>;
  constexpr int CB = Map::CB, CW = CB * DEXSIM_NJ, TIN = (64 * CW + KD_THREADS - 1) / KD_THREADS;
  __shared__ float s_w[Map::WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;

  float tin[TIN];

  // ---- setup: the walk, the bias force (FD), the finger's blocks and their elimination
  float qb[6], qf[4];
  const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
  KinBase B;
  kd_base_walk(P, qb, B);
  if (f == 0) s_valid[lane] = valid;

  float cf[4] = {0.f, 0.f, 0.f, 0.f};   // FD: bias force of the finger's joints
  V3 a[4], o[4];
  Comp comp[4];
  {
    V3 fl[4], nl[4];
    float vf[4] = {0.f, 0.f, 0.f, 0.f};
    KdMotion m = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};
    if (FD) {
      float vb[6];
      kd_load_qd(A, K.rows, K.qd, N, NR, f, vb, vf);
      const V3 g = v3p(P->cfg.gravity);
      KdMotion mb[6];
      kd_base_motion(B, vb, nullptr, K.gravity ? v3(-g.x, -g.y, -g.z) : v3(0, 0, 0), mb);
      m = mb[5];
      if (f == 0) {   // for the palm pass, through LDS: nine registers less from here to there
        KD_PUT3(Map::M5, m.w); KD_PUT3(Map::M5 + 3, m.al); KD_PUT3(Map::M5 + 6, m.ao);
      }
    }
    V3 of = v3(0, 0, 0), op = v3(0, 0, 0);
    Q4 qc = B.q[5];
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) {
      const JC& c = P->jc[6 + 4 * f + l];
      kd_finger_joint(c, qf[l], of, qc, a[l]);   // kd_finger_link spelled out: through it the mass solve was 2 to 7 % slower
      o[l] = of;
      const M3 Rj = q2mat(qc);
      const V3 rc = fd_opaque(mul(Rj, v3p(c.com)));
      const S6 I = fd_opaque(rotate_inertia(Rj, c.inertia));
      comp[l].m = c.mass; comp[l].c = of + rc; comp[l].I = I;
      if (FD) {
        m = kd_joint_motion(m, of - op, a[l], vf[l], 0.f, false);
        op = of;
        kd_link_wrench(c.mass, rc, I, m, fl[l], nl[l]);
        __builtin_amdgcn_sched_barrier(0);   // link by link: interleaved for ILP, four links' inertias and wrenches do not fit the registers
      }
    }
    if (FD) kd_finger_backward(a, o, fl, nl, cf, 1, s_w, Map::WR + 6 * f, lane);
  }
  // the scheduler interleaves for ILP and would start the composites inside the walk: the two together do not fit the registers
  __builtin_amdgcn_sched_barrier(0);
  if (FD) fd_cols_load<CW, TIN>(K, 0, tin);   // tau is on its way during the composites and the elimination
#pragma unroll
  for (int l = DEXSIM_NFJ - 2; l >= 0; l--) comp_add(comp[l], comp[l + 1]);   // subtree of joint l = links l .. 3
  float Fm[16], Cm[24], G[24];   // F_f (then its inverse), C_f as Cm[6 i + k]: finger joint i, base joint k; G[6 l + k]
#pragma unroll
  for (int i = 0; i < DEXSIM_NFJ; i++) {
    const V3 Pm = comp[i].m * cross(a[i], comp[i].c - o[i]);
    const V3 L = mul(comp[i].I, a[i]);
#pragma unroll
    for (int k = 0; k <= i; k++) { const float v = dot(a[k], L + cross(comp[i].c - o[k], Pm)); Fm[4 * i + k] = v; Fm[4 * k + i] = v; }
#pragma unroll
    for (int k = 0; k < 6; k++) Cm[6 * i + k] = k < 3 ? dot(B.a[k], Pm) : dot(B.a[k], L + cross(comp[i].c - B.orel[k], Pm));
  }
  if (K.armature) {
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) Fm[5 * l] += P->jc[6 + 4 * f + l].armature;
  }
  spd_inverse<4>(Fm);
#pragma unroll
  for (int l = 0; l < DEXSIM_NFJ; l++)
#pragma unroll
    for (int k = 0; k < 6; k++) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < DEXSIM_NFJ; i++) s += Fm[4 * l + i] * Cm[6 * i + k];
      G[6 * l + k] = s;
    }
  {
    float Bf[21];
    kd_base_block(B, comp[0], Bf);
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int k = 0; k <= i; k++) {
        float s = 0.f;
#pragma unroll
        for (int l = 0; l < DEXSIM_NFJ; l++) s += Cm[6 * l + i] * G[6 * l + k];
        s_w[(Map::SCH + 21 * f + KD_TRI(i, k)) * KD_LD + lane] = Bf[KD_TRI(i, k)] - s;
      }
  }
  if (FD) fd_cols_stage<CW, TIN>(s_w, Map::STAGE, tin);
  __syncthreads();
  if (!FD) fd_cols_load<CW, TIN>(K, 0, tin);   // the first batch (up to 21 registers) flies during the factor: the walk's registers are free

  // ---- factor (wave 0): the palm link's block, the five finger parts, the armature; FD: the palm pass of the bias force
  float L6[21], rd[6], cB[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (f == 0) {
    const JC& c5 = P->jc[5];
    const M3 R5 = q2mat(B.q[5]);
    Comp H;
    H.m = c5.mass; H.c = fd_opaque(mul(R5, v3p(c5.com))); H.I = fd_opaque(rotate_inertia(R5, c5.inertia));
    float S[21];
    kd_base_block(B, H, S);
#pragma unroll
    for (int ff = 0; ff < DEXSIM_NFINGER; ff++)
#pragma unroll
      for (int i = 0; i < 21; i++) S[i] += s_w[(Map::SCH + 21 * ff + i) * KD_LD + lane];
    if (K.armature) {
#pragma unroll
      for (int i = 0; i < 6; i++) S[KD_TRI(i, i)] += P->jc[i].armature;
    }
    fd_chol6(S, L6, rd);
    if (FD) {
      V3 F, Nm;
      const float* const w5 = s_w + Map::M5 * KD_LD + lane;
      const KdMotion m5 = {v3(w5[0], w5[KD_LD], w5[2 * KD_LD]), v3(w5[3 * KD_LD], w5[4 * KD_LD], w5[5 * KD_LD]),
                           v3(w5[6 * KD_LD], w5[7 * KD_LD], w5[8 * KD_LD])};
      kd_link_wrench(c5.mass, H.c, H.I, m5, F, Nm);
      kd_palm_project(B, F, Nm, s_w, Map::WR, lane, cB, 1);
    }
  }
  if (!FD) {
    fd_cols_stage<CW, TIN>(s_w, Map::STAGE, tin);
    __syncthreads();   // the batch is staged; and CFR lies over SCH, which wave 0 has read
  }

  // ---- the columns
  for (int c0 = 0;;) {
    const int nc = min(CB, K.nrhs - c0);
#pragma unroll
    for (int cc = 0; cc < CB; cc++) {   // fingers: y_f = F_f^-1 r_f in place, G_f^T r_f
      if (cc >= nc) break;
      float* const w = s_w + (Map::STAGE + DEXSIM_NJ * cc + 6 + 4 * f) * KD_LD + lane;
      float r[4];
#pragma unroll
      for (int l = 0; l < DEXSIM_NFJ; l++) { r[l] = w[l * KD_LD]; if (FD) r[l] -= cf[l]; r[l] = opaque(r[l]); }
#pragma unroll
      for (int l = 0; l < DEXSIM_NFJ; l++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < DEXSIM_NFJ; i++) s += Fm[4 * l + i] * r[i];
        w[l * KD_LD] = s;
      }
#pragma unroll
      for (int k = 0; k < 6; k++) {
        float s = 0.f;
#pragma unroll
        for (int l = 0; l < DEXSIM_NFJ; l++) s += G[6 * l + k] * r[l];
        s_w[(Map::CFR + 6 * (DEXSIM_NFINGER * cc + f) + k) * KD_LD + lane] = s;
      }
    }
    __syncthreads();
    if (f == 0) {   // wave 0: x_B in place
#pragma unroll
      for (int cc = 0; cc < CB; cc++) {
        if (cc >= nc) break;
        float* const w = s_w + (Map::STAGE + DEXSIM_NJ * cc) * KD_LD + lane;
        float rb[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { rb[i] = w[i * KD_LD]; if (FD) rb[i] -= cB[i]; rb[i] = opaque(rb[i]); }
#pragma unroll
        for (int ff = 0; ff < DEXSIM_NFINGER; ff++)
#pragma unroll
          for (int i = 0; i < 6; i++) rb[i] -= s_w[(Map::CFR + 6 * (DEXSIM_NFINGER * cc + ff) + i) * KD_LD + lane];
        fd_chol6_solve(L6, rd, rb, x);
#pragma unroll
        for (int i = 0; i < 6; i++) w[i * KD_LD] = x[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int cc = 0; cc < CB; cc++) {   // fingers: x_f = y_f - G_f x_B in place
      if (cc >= nc) break;
      float* const w = s_w + (Map::STAGE + DEXSIM_NJ * cc) * KD_LD + lane;
      float xb[6];
#pragma unroll
      for (int i = 0; i < 6; i++) xb[i] = w[i * KD_LD];
#pragma unroll
      for (int l = 0; l < DEXSIM_NFJ; l++) {
        float s = w[(6 + 4 * f + l) * KD_LD];
#pragma unroll
        for (int k = 0; k < 6; k++) s -= G[6 * l + k] * xb[k];
        w[(6 + 4 * f + l) * KD_LD] = s;
      }
    }
    __syncthreads();
    if (FD) { kd_flush<false>(s_w, s_valid, Map::STAGE, DEXSIM_NJ, K.out); break; }
    kd_flush<false, CW>(s_w, s_valid, Map::STAGE, min(CW, (K.nrhs - c0) * DEXSIM_NJ), K.out, (size_t)K.nrhs * DEXSIM_NJ, (size_t)c0 * DEXSIM_NJ);
    c0 += CB;
    if (c0 >= K.nrhs) break;
    fd_cols_load<CW, TIN>(K, c0, tin);   // (issued at the head of the batch before, these loads made the call slower: README of the profile)
    __syncthreads();   // the flush has read the batch
    fd_cols_stage<CW, TIN>(s_w, Map::STAGE, tin);
    __syncthreads();
  }
}
