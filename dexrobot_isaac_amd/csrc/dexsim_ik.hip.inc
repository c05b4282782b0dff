// dexsim_ik.hip.inc -- batched inverse kinematics of the five fingertips (or fingerpads) in CONTROL space (dexsim_solve_ik): damped
// least squares on the 18 active targets of the action stage, every iteration inside one launch.  Not on the step path; reads q
// (arena rows or the caller's override) and the model, writes caller-owned memory only.
//
// The workgroup is that of dexsim_chain.hip.inc: 64 rows x 5 waves, wave f walks finger f, o5-relative positions, [word][row] LDS,
// a `valid` flag per row that only gates stores.  Plain __syncthreads() only: no atomics, no spins.
//
// A finger's site moves with at most 9 controls, its LOCAL columns: 0-5 the base controls, 6 its "spread" control (control 6 for
// the thumb, the shared control 9 for index, ring and pinky -- the pinky's DOF turns twice as far --, none for the middle finger,
// whose spread DOF 14 is held at 0), 7 its MCP control and 8 its DIP control (two DOFs, one control: the column is the sum of the
// two joint columns).  MCP and DIP are PRIVATE to the finger: in A = sum_f w_f J_f^T J_f + l^2 I they couple to nothing but the
// finger's own seven other columns.  The 18 x 18 Cholesky factorisation therefore runs in the elimination order "the ten private
// controls first, then the eight SHARED ones (0-5, 6, 9)", in which it has no fill-in and splits over the waves:
//   every wave   walks its chain at q(u), forms e_f = t_f - p_f, the 3 x 9 Jacobian and H = w_f J^T J, g = w_f J^T e; factorises its
//                private 2 x 2 block, and leaves its Schur complement on the shared columns (7 x 7 lower triangle + 7) in LDS
//   barrier
//   wave 0       one row per lane, in registers: sums the five complements in the order f = 0..4 into the 8 x 8 shared system, adds
//                l^2, factorises and solves it; the shared steps go to LDS
//   barrier
//   every wave   back-substitutes its two private steps, to LDS
//   barrier
//   every wave   the step limit over all 18 steps and the clamped update of the nine controls IT uses, in registers: the waves
//                that share a control compute the same bits from the same words
// A fixed control is an identity row with a zero right-hand side: its step is an exact 0.  A row's result is a function of that
// row alone.  After the last iteration every wave evaluates its site once more for the residual, and the workgroup flushes
// controls, q_out and residual from LDS along the contiguous output index.

#define IK_NLOC 9                                   /* local columns of a finger: 6 base, spread, MCP, DIP */
#define IK_NSH 7                                    /* of which shared (local 0..6) */
#define IK_TRI(i, j) ((i) * ((i) + 1) / 2 + (j))    /* lower triangle, j <= i */
#define IK_BLK (IK_NSH * (IK_NSH + 1) / 2 + IK_NSH) /* a finger's Schur complement: 28 + 7 words */
#define IK_U 0                                      /* [18] start value, later the result */
#define IK_D DEXSIM_NACT                            /* [18] the step */
#define IK_B(f) (2 * DEXSIM_NACT + (f) * IK_BLK)    /* complement of finger f */
#define IK_WORDS (2 * DEXSIM_NACT + DEXSIM_NFINGER * IK_BLK)
#define IK_Q IK_B(0)                                /* after the loop, over the complements: [26] q_out, [5] residual */
#define IK_RES (IK_Q + DEXSIM_NJ)
// The library is built with the scheduler's max-ILP strategy for the step kernel; here it would interleave the whole iteration and
// run out of registers.  A fence between the stages keeps each stage's temporaries to itself.
#define IK_STAGE() __builtin_amdgcn_sched_barrier(0)
#define IK_NSYS 8                                   /* shared system: controls 0-5, 6, 9 */
static_assert(IK_RES + DEXSIM_NFINGER <= IK_WORDS, "k_ik_solve: the output staging does not fit over the complements");
static_assert(IK_WORDS * KD_LD * 4 + 256 <= 65536, "k_ik_solve: static LDS above 64 KiB");
static_assert(DEXSIM_NACT == 18 && DEXSIM_NFINGER == 5 && DEXSIM_NFJ == 4, "k_ik_solve is written for the 18 controls of kCoupling");

// control of local column 6 + s of finger f (s = 0 spread, 1 MCP, 2 DIP); -1: the middle finger has no spread control
__host__ DI constexpr int ik_control(int f, int s) {
  return s == 0 ? (f == 0 ? 6 : f == 2 ? -1 : 9) : (f == 0 ? 6 + s : f == 1 ? 9 + s : f == 2 ? 11 + s : f == 3 ? 13 + s : 15 + s);
}
// scale of the finger's first DOF on its spread control
__host__ DI constexpr float ik_spread_scale(int f) { return f == 2 ? 0.f : f == 4 ? 2.f : 1.f; }
// the finger whose first DOF is the first of its spread group: that DOF gives the control its start value, that wave stores it
__host__ DI constexpr bool ik_spread_first(int f) { return f <= 1; }

// control of row i of the shared system: the base controls, then the spread controls in the order of their first fingers
__host__ DI constexpr int ik_sys_control(int i) { return i < 6 ? i : ik_control(i - 6, 0); }
static_assert(IK_NSYS == 8 && ik_spread_first(0) && ik_spread_first(1), "the shared system's rows 6 and 7 are the thumb's and the index's spread control");
// row of the shared system that local column i (< IK_NSH) of finger ff lands on (-1: the middle finger's empty spread column)
__host__ DI constexpr int ik_sys_row(int ff, int i) {
  const int c = i < 6 ? i : ik_control(ff, 0);
  for (int r = 0; r < IK_NSYS; r++) if (ik_sys_control(r) == c) return r;
  return -1;
}

// The table above IS kCoupling, read finger by finger: checked here so that the two cannot drift apart.
constexpr bool ik_table_matches_coupling() {
  for (int f = 0; f < 5; f++) {
    const int d0 = 6 + 4 * f;
    const int cs = ik_control(f, 0), cm = ik_control(f, 1), cd = ik_control(f, 2);
    if (cs < 0) { if (d0 != kHeldDof) return false; }
    else {
      bool hit = false;
      for (int i = 0; i < kCoupling[cs].n; i++) hit = hit || (kCoupling[cs].dof[i] == d0 && kCoupling[cs].scale[i] == ik_spread_scale(f));
      if (!hit || ik_spread_first(f) != (kCoupling[cs].dof[0] == d0)) return false;
    }
    if (kCoupling[cm].n != 1 || kCoupling[cm].dof[0] != d0 + 1 || kCoupling[cm].scale[0] != 1.f) return false;
    if (kCoupling[cd].n != 2 || kCoupling[cd].dof[0] != d0 + 2 || kCoupling[cd].dof[1] != d0 + 3 || kCoupling[cd].scale[0] != 1.f ||
        kCoupling[cd].scale[1] != 1.f) return false;
  }
  for (int c = 0; c < 6; c++) if (kCoupling[c].n != 1 || kCoupling[c].dof[0] != c) return false;
  return true;
}
static_assert(ik_table_matches_coupling(), "k_ik_solve: the per-finger control table differs from kCoupling");

struct IkArgs {
  KinRows rows;
  const float* targets;   // (k, 5, 3)
  float* controls;        // (k, 18)
  float* q_out;           // (k, 26) or NULL
  float* residual;        // (k, 5) or NULL
  DexSimIK prm;
  float lam2;             // damping^2
};

// q(u) of the finger's chain from its nine local controls u, the residual e = t - p and the nine local Jacobian columns
struct IkEval { V3 e; V3 J[IK_NLOC]; float qf[4]; };

template <bool kJac>
DI void ik_eval(const DevParams* __restrict__ P, const float* u, int f, int site, int frame, V3 tgt, IkEval& E) {
  const DexHandModel& M = P->model;
  const float sc = ik_spread_scale(f);
  E.qf[0] = ik_control(f, 0) < 0 ? 0.f : sc * u[6];   // kHeldDof: +0.0f
  E.qf[1] = u[7];
  E.qf[2] = E.qf[3] = u[8];
  KinBase B;
  kd_base_walk(P, u, B);
  IK_STAGE();
  V3 of = v3(0, 0, 0), a[4], o[4];
  Q4 qc = B.q[5];
#pragma unroll
  for (int l = 0; l < DEXSIM_NFJ; l++) {
    kd_finger_joint(P->jc[6 + 4 * f + l], E.qf[l], of, qc, a[l]);
    o[l] = of;
  }
  IK_STAGE();
  const V3 p = of + mul(q2mat(qc), v3p(M.site_p[site]));
  if (frame == 0) {   // world target: o5 = o0 - orel[0], o0 from the spawn frame and the first slide
    const V3 o0 = v3p(M.spawn_pos) + mul(q2mat(q4p(M.spawn_quat)), v3p(P->jc[0].poff)) + u[0] * B.a[0];
    E.e = (tgt - (o0 - B.orel[0])) - p;
  } else {
    E.e = tgt - p;    // already relative to o5 (k_ik_solve maps a hand-frame target once, the base is fixed)
  }
  if (kJac) {
#pragma unroll
    for (int j = 0; j < 6; j++) E.J[j] = j < 3 ? B.a[j] : cross(B.a[j], p - B.orel[j]);
    E.J[6] = sc * cross(a[0], p - o[0]);
    E.J[7] = cross(a[1], p - o[1]);
    E.J[8] = cross(a[2], p - o[2]) + cross(a[3], p - o[3]);
  }
}

// x = A^-1 b for an SPD n x n matrix (lower triangle in IK_TRI order, overwritten by its Cholesky factor); fully unrolled
template <int n>
DI void ik_chol_solve(float* A, const float* b, float* x) {
  float rd[n];
#pragma unroll
  for (int i = 0; i < n; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) {
      float s = A[IK_TRI(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) s -= A[IK_TRI(i, k)] * A[IK_TRI(j, k)];
      if (i == j) { const float d = sqrtf(fmaxf(s, 1e-30f)); A[IK_TRI(i, i)] = d; rd[i] = 1.f / d; }
      else A[IK_TRI(i, j)] = s * rd[j];
    }
#pragma unroll
  for (int i = 0; i < n; i++) {
    float s = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) s -= A[IK_TRI(i, k)] * x[k];
    x[i] = s * rd[i];
  }
#pragma unroll
  for (int i = n - 1; i >= 0; i--) {
    float s = x[i];
#pragma unroll
    for (int k = i + 1; k < n; k++) s -= A[IK_TRI(k, i)] * x[k];
    x[i] = s * rd[i];
  }
}

template <int ff>
DI void ik_add_complement(float* A, float* b, const float* src) {
#pragma unroll
  for (int i = 0; i < IK_NSH; i++) {
    const int gi = ik_sys_row(ff, i);
    if (gi < 0) continue;
#pragma unroll
    for (int j = 0; j <= i; j++) A[IK_TRI(gi, ik_sys_row(ff, j))] += src[IK_TRI(i, j) * KD_LD];
    b[gi] += src[(IK_NSH * (IK_NSH + 1) / 2 + i) * KD_LD];
  }
}

__global__ __launch_bounds__(KD_THREADS) void k_ik_solve(const DevParams* __restrict__ P, IkArgs K, int N, int NR) {
  __shared__ float s_w[IK_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const DexSimConfig& C = P->cfg;
  const DexHandModel& M = P->model;
  const int site = (K.prm.sites ? 6 : 1) + f, frame = K.prm.frame;
  const unsigned free_mask = K.prm.free_mask;
  const int row = min(blockIdx.x * 64 + lane, K.rows.k - 1);   // every lane reads a legal address
  // the controls of the wave's local columns (wave-uniform); an empty column (the middle finger's spread) is never free and its u
  // is not used: it reads control 0, a legal index
  int ctl[IK_NLOC];
  bool fr[IK_NLOC];
  float lo[IK_NLOC], hi[IK_NLOC];
#pragma unroll
  for (int i = 0; i < IK_NLOC; i++) {
    const int c = i < 6 ? i : ik_control(f, i - 6);
    ctl[i] = max(c, 0);
    fr[i] = ((free_mask >> ctl[i]) & 1u) != 0 && c >= 0;
    lo[i] = C.active_lower[ctl[i]]; hi[i] = C.active_upper[ctl[i]];
  }

  {   // ---- start value: u0_c = clamp(q0[first DOF of group c]); every wave the controls it owns (control 9 belongs to the index)
    float qb[6], qf[4];
    const bool valid = kd_load_q(A, K.rows, N, NR, f, qb, qf);
    if (f == 0) {
      s_valid[lane] = valid;
#pragma unroll
      for (int j = 0; j < 6; j++) s_w[(IK_U + j) * KD_LD + lane] = clampf(qb[j], lo[j], hi[j]);
    }
    if (ik_spread_first(f)) s_w[(IK_U + ctl[6]) * KD_LD + lane] = clampf(qf[0], lo[6], hi[6]);
    s_w[(IK_U + ctl[7]) * KD_LD + lane] = clampf(qf[1], lo[7], hi[7]);
    s_w[(IK_U + ctl[8]) * KD_LD + lane] = clampf(qf[2], lo[8], hi[8]);
  }
  __syncthreads();
  float u[IK_NLOC];
#pragma unroll
  for (int i = 0; i < IK_NLOC; i++) u[i] = s_w[(IK_U + ctl[i]) * KD_LD + lane];

  const size_t t0 = ((size_t)row * DEXSIM_NFINGER + f) * 3;
  V3 tgt = v3(GPTR(K.targets)[t0], GPTR(K.targets)[t0 + 1], GPTR(K.targets)[t0 + 2]);
  if (frame == 1) {   // hand frame -> relative to o5, through the pose of site 0 at u0 (the base is fixed in this mode)
    KinBase B;
    kd_base_walk(P, u, B);
    tgt = mul(q2mat(B.q[5]), v3p(M.site_p[0])) + mul(q2mat(qmul(B.q[5], q4p(M.site_q[0]))), tgt);
  }
  const float wf = K.prm.weight[f];
  float* const s_b = s_w + IK_B(f) * KD_LD + lane;   // the wave's complement

  for (int it = 0; it < K.prm.iters; it++) {
    // the private 2 x 2 block D = L L^T, Y = E L^-T (the shared columns' coupling to it), z = L^-1 g_D
    float y1[IK_NSH], y2[IK_NSH], z1, z2, r1, r2, l21;
    {
      IkEval E;
      ik_eval<true>(P, u, f, site, frame, tgt, E);
      IK_STAGE();
      V3 wJ[IK_NLOC];
#pragma unroll
      for (int i = 0; i < IK_NLOC; i++) wJ[i] = fr[i] ? wf * E.J[i] : v3(0, 0, 0);   // a fixed control: zero row and column
      const float d11 = fr[7] ? dot(wJ[7], E.J[7]) + K.lam2 : 1.f, d22 = fr[8] ? dot(wJ[8], E.J[8]) + K.lam2 : 1.f;
      const float d21 = fr[7] ? dot(wJ[8], E.J[7]) : 0.f;
      r1 = 1.f / sqrtf(d11);
      l21 = d21 * r1;
      r2 = 1.f / sqrtf(fmaxf(d22 - l21 * l21, 1e-30f));
      z1 = dot(wJ[7], E.e) * r1;
      z2 = (dot(wJ[8], E.e) - l21 * z1) * r2;
#pragma unroll
      for (int i = 0; i < IK_NSH; i++) {
        y1[i] = fr[7] ? dot(wJ[i], E.J[7]) * r1 : 0.f;
        y2[i] = ((fr[8] ? dot(wJ[i], E.J[8]) : 0.f) - y1[i] * l21) * r2;
      }
      IK_STAGE();
#pragma unroll
      for (int i = 0; i < IK_NSH; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) s_b[IK_TRI(i, j) * KD_LD] = (fr[j] ? dot(wJ[i], E.J[j]) : 0.f) - y1[i] * y1[j] - y2[i] * y2[j];
        s_b[(IK_NSH * (IK_NSH + 1) / 2 + i) * KD_LD] = dot(wJ[i], E.e) - y1[i] * z1 - y2[i] * z2;
      }
    }
    __syncthreads();
    if (f == 0) {   // ---- the shared system: controls 0-5, 6, 9
      float As[IK_NSYS * (IK_NSYS + 1) / 2], bs[IK_NSYS], xs[IK_NSYS];
#pragma unroll
      for (int i = 0; i < IK_NSYS * (IK_NSYS + 1) / 2; i++) As[i] = 0.f;
#pragma unroll
      for (int i = 0; i < IK_NSYS; i++) bs[i] = 0.f;
      const float* const src = s_w + lane;
      ik_add_complement<0>(As, bs, src + IK_B(0) * KD_LD);
      ik_add_complement<1>(As, bs, src + IK_B(1) * KD_LD);
      ik_add_complement<2>(As, bs, src + IK_B(2) * KD_LD);
      ik_add_complement<3>(As, bs, src + IK_B(3) * KD_LD);
      ik_add_complement<4>(As, bs, src + IK_B(4) * KD_LD);
#pragma unroll
      for (int i = 0; i < IK_NSYS; i++) {
        const bool fi = (free_mask >> ik_sys_control(i)) & 1u;
        As[IK_TRI(i, i)] = fi ? As[IK_TRI(i, i)] + K.lam2 : 1.f;
      }
      ik_chol_solve<IK_NSYS>(As, bs, xs);
#pragma unroll
      for (int i = 0; i < IK_NSYS; i++) s_w[(IK_D + ik_sys_control(i)) * KD_LD + lane] = xs[i];
    }
    __syncthreads();
    {   // ---- the private steps: d_D = L^-T (z - Y^T d_S)
      float t1 = z1, t2 = z2;
#pragma unroll
      for (int i = 0; i < IK_NSH; i++) {
        const float ds = (i == 6 && ik_control(f, 0) < 0) ? 0.f : s_w[(IK_D + ctl[i]) * KD_LD + lane];
        t1 -= y1[i] * ds; t2 -= y2[i] * ds;
      }
      const float d8 = t2 * r2, d7 = (t1 - l21 * d8) * r1;
      s_w[(IK_D + ctl[7]) * KD_LD + lane] = d7;
      s_w[(IK_D + ctl[8]) * KD_LD + lane] = d8;
    }
    __syncthreads();
    {   // ---- s = min(1, max_step / max |d|), u <- clamp(u + s d)
      float m = 0.f;
#pragma unroll
      for (int c = 0; c < DEXSIM_NACT; c++) m = fmaxf(m, fabsf(s_w[(IK_D + c) * KD_LD + lane]));
      const float s = m > K.prm.max_step ? K.prm.max_step / m : 1.f;
#pragma unroll
      for (int i = 0; i < IK_NLOC; i++)
        if (fr[i]) u[i] = clampf(u[i] + s * s_w[(IK_D + ctl[i]) * KD_LD + lane], lo[i], hi[i]);
    }
  }

  {   // ---- final evaluation: residual, u and q(u), staged over the complements (every wave is past its last read of them)
    IkEval E;
    ik_eval<false>(P, u, f, site, frame, tgt, E);
    s_w[(IK_RES + f) * KD_LD + lane] = sqrtf(dot(E.e, E.e));
#pragma unroll
    for (int l = 0; l < DEXSIM_NFJ; l++) s_w[(IK_Q + 6 + 4 * f + l) * KD_LD + lane] = E.qf[l];
    if (f == 0) {
#pragma unroll
      for (int j = 0; j < 6; j++) { s_w[(IK_Q + j) * KD_LD + lane] = u[j]; s_w[(IK_U + j) * KD_LD + lane] = u[j]; }
    }
    if (ik_spread_first(f)) s_w[(IK_U + ctl[6]) * KD_LD + lane] = u[6];
    s_w[(IK_U + ctl[7]) * KD_LD + lane] = u[7];
    s_w[(IK_U + ctl[8]) * KD_LD + lane] = u[8];
  }
  __syncthreads();

  kd_flush<false>(s_w, s_valid, IK_U, DEXSIM_NACT, K.controls);
  if (K.q_out) kd_flush<false>(s_w, s_valid, IK_Q, DEXSIM_NJ, K.q_out);
  if (K.residual) kd_flush<false>(s_w, s_valid, IK_RES, DEXSIM_NFINGER, K.residual);
}
