// dexsim_proximity.hip.inc -- clearance queries of the hand (dexsim_query_proximity): every collision capsule against the box and
// the ground plane, and the capsules of different fingers (and of the palm) against each other.  A pure function of q and the box
// pose, like the camera and the kinematics tensors: one kernel, not on the step path; it reads q (arena rows or the caller's
// override) and the box pose (arena rows or the caller's) and writes caller-owned memory only.
//
// One workgroup in the shape of dexsim_chain.hip.inc (64 rows x 5 waves, [word][row] LDS, o5-relative positions):
//   phase A  the scene stage of dexsim_chain.hip.inc (KD_PLACE_HAND): the axis ends of the capsules relative to o5, and o5 (world),
//            in LDS.  Every hand-internal difference of phase B is therefore a difference of numbers of hand size (< 0.4 m), not of
//            world coordinates, and the box (KD_LOAD_BOX) enters through (o5 - centre) alone.
//   phase B  lanes stay on the rows.  Wave w takes the finger groups 2 w and 2 w + 1 and the palm group 10 + w (9 + 9 + 6 = 24
//            segment pairs) and the environment records of the capsules w, w + 5, w + 10, w + 15.  The loops are fully unrolled and
//            the pairs of a group do not depend on each other (only the strict-less minimum chains them), so the scheduler
//            interleaves their chains: a lone wave issues a dependent instruction only every few cycles (collide_capsules3).
//            Records leave as two 16-byte stores per lane; pair_dist goes through LDS and leaves as contiguous 16-byte stores of
//            all five waves (phase C, kd_flush).
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.
//
// Geometry (the contract is in include/dexsim.h):
//   capsule / box      the closest point of the axis to the cube in CLOSED FORM: with P(t) = a + t d in the cube's frame and
//                      f(t) = |P - clamp(P)|^2, f' is piecewise linear and non-decreasing with breakpoints where a coordinate
//                      crosses +-hb.  f' is evaluated at 0, 1 and the six (clamped) breakpoints; the largest t with f' < 0 and the
//                      smallest with f' >= 0 bracket a piece on which f' is linear: one interpolation gives the minimiser, and the
//                      start of a flat stretch (always a breakpoint, or 0) when the minimum is not unique.  No iteration, no
//                      branch.  The distance itself is sphere_box (dexsim_device.h) at that point, or, where the axis
//                      meets the cube, at the midpoint of the stretch inside it (slab clipping).
//   capsule / capsule  clamped closest points of two segments, the standard two-stage clamping.

#define DEXSIM_PX_ZERO_AXIS2 1e-18f   /* |axis|^2 below this: the capsule is a sphere (axis shorter than 1e-9 m) */

#define PX_CAP 0                               /* [DEXSIM_NCAP][6] axis ends p0.xyz p1.xyz relative to o5 */
#define PX_O5 (6 * DEXSIM_NCAP)                /* [3] o5, world */
#define PX_PD (PX_O5 + 3)                      /* [DEXSIM_NPROX_PAIRS] pair distances on their way to phase C */
#define PX_WORDS (PX_PD + DEXSIM_NPROX_PAIRS)
static_assert(DEXSIM_NPROX_PAIRS == 10 * 9 + 5 * 6 && DEXSIM_NPROX_GROUPS == 15, "pair table: 10 finger groups of 9, 5 palm groups of 6");
static_assert(DEXSIM_NPROX_PAIRS % 4 == 0, "pair_dist rows are written as 16-byte quads");
static_assert(PX_WORDS * KD_LD * 4 + 256 <= 65536, "k_proximity: static LDS above 64 KiB");

// finger pair (fa < fb) of group g = 0..9, lexicographic: (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4)
__host__ DI int px_group_fa(int g) { return (int)((0x3221110000ull >> (4 * g)) & 15); }
__host__ DI int px_group_fb(int g) { return (int)((0x4434324321ull >> (4 * g)) & 15); }

struct ProxArgs {
  KinRows rows;
  KinBox box;
  float* cap_env;          // (k, DEXSIM_NCAP, 2, 8) or NULL
  float* self_min;         // (k, DEXSIM_NPROX_GROUPS, 8) or NULL
  float* pair_dist;        // (k, DEXSIM_NPROX_PAIRS) or NULL
};

DI float px_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // a NaN becomes 0
// per-component select: `c ? a : b` on a struct is a select of addresses and puts both operands in scratch
DI V3 px_sel(bool c, V3 a, V3 b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }

// Capsule axis P(t) = a + t d (cube frame), radius r, against the solid cube of half edge hb: local normal, witness on the cube,
// signed distance and the axis parameter of the witness.
DI void px_capsule_box(V3 a, V3 d, float r, float hb, V3& nl, V3& pl, float& dist, float& tw) {
  const float av[3] = {a.x, a.y, a.z}, dv[3] = {d.x, d.y, d.z};
  float tk[6];
  float tin = 0.f, tout = 1.f;   // the stretch of the axis inside the cube (empty: tin > tout)
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const bool mv = fabsf(dv[i]) > 1e-30f;   // the quotients below stay finite: numerators are of scene size
    const float inv = 1.f / (mv ? dv[i] : 1.f);
    const float t1 = (-hb - av[i]) * inv, t2 = (hb - av[i]) * inv;
    tk[2 * i] = mv ? px_clamp01(t1) : 0.f;
    tk[2 * i + 1] = mv ? px_clamp01(t2) : 0.f;
    const bool out = fabsf(av[i]) > hb;
    tin = mv ? fmaxf(tin, fminf(t1, t2)) : (out ? 2.f : tin);
    tout = mv ? fminf(tout, fmaxf(t1, t2)) : (out ? -1.f : tout);
  }
  const float g0 = seg_box_dfdt(a, d, 0.f, hb), g1 = seg_box_dfdt(a, d, 1.f, hb);
  float tl = 0.f, gl = g0, th = 1.f, gh = g1;   // bracket of the sign change of f' (meaningful when g0 < 0 <= g1)
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float g = seg_box_dfdt(a, d, tk[k], hb);
    const bool lo = g < 0.f && tk[k] > tl, hi = g >= 0.f && tk[k] < th;
    tl = lo ? tk[k] : tl; gl = lo ? g : gl;
    th = hi ? tk[k] : th; gh = hi ? g : gh;
  }
  const float den = gh - gl;   // > 0 inside the bracket
  const float troot = fminf(fmaxf(tl + (th - tl) * (-gl / (den > 0.f ? den : 1.f)), tl), th);
  const float ts = g0 >= 0.f ? 0.f : (g1 < 0.f ? 1.f : troot);
  const V3 Ps = {a.x + ts * d.x, a.y + ts * d.y, a.z + ts * d.z};
  const V3 ex = {Ps.x - clampf(Ps.x, -hb, hb), Ps.y - clampf(Ps.y, -hb, hb), Ps.z - clampf(Ps.z, -hb, hb)};
  const bool meets = !(dot(ex, ex) > 1e-12f);   // sphere_box's own threshold: its inside branch
  tw = (meets && tin <= tout) ? 0.5f * (tin + tout) : ts;
  const V3 Pw = {a.x + tw * d.x, a.y + tw * d.y, a.z + tw * d.z};
  sphere_box(Pw, r, hb, nl, pl, dist);
}

// clamped closest points p1 + s d1, p2 + t d2 of two segments (two-stage clamping; parallel axes: s = 0; a zero-length axis is a point)
DI void px_seg_seg(V3 r, V3 d1, V3 d2, float& s, float& t) {   // r = p1 - p2
  const float a = dot(d1, d1), e = dot(d2, d2), b = dot(d1, d2), c = dot(d1, r), f = dot(d2, r);
  const bool za = !(a > DEXSIM_PX_ZERO_AXIS2), ze = !(e > DEXSIM_PX_ZERO_AXIS2);
  const float ae = a * e, den = ae - b * b;
  const bool par = za || ze || !(den > 1e-12f * ae);
  const float s1 = par ? 0.f : px_clamp01((b * f - c * e) / (par ? 1.f : den));
  const float traw = ze ? 0.f : (b * s1 + f) / (ze ? 1.f : e);
  t = px_clamp01(traw);
  const float s2 = za ? 0.f : px_clamp01((b * t - c) / (za ? 1.f : a));
  s = (ze || traw != t) ? s2 : s1;
}

struct PxSeg { V3 p, d; float r; };   // axis start relative to o5, axis, radius

DI PxSeg px_load_seg(const float* s_w, int lane, const DexHandModel& M, int cap) {
  const float* const w = s_w + (PX_CAP + 6 * cap) * KD_LD + lane;
  PxSeg S;
  S.p = v3(w[0], w[KD_LD], w[2 * KD_LD]);
  S.d = v3(w[3 * KD_LD], w[4 * KD_LD], w[5 * KD_LD]) - S.p;
  S.r = M.cap_r[cap];
  return S;
}

// One group: the capsules capA[0..3) against capB[0..NB), pair index pair0 + la * NB + lb.  Leaves every distance in LDS (want_pd)
// and the closest pair's record in rec[8] (ties: the lowest pair index).
template <int NB>
DI void px_group(float* s_w, int lane, const DexHandModel& M, const int (&capA)[3], const int (&capB)[3], int pair0, V3 o5, bool want_pd,
                 float (&rec)[8]) {
  PxSeg B[NB];
#pragma unroll
  for (int lb = 0; lb < NB; lb++) B[lb] = px_load_seg(s_w, lane, M, capB[lb]);
  float best = 0.f;
  V3 bn = v3(0, 0, 1), bp = v3(0, 0, 0);
  int bi = pair0;
#pragma unroll
  for (int la = 0; la < 3; la++) {
    const PxSeg A = px_load_seg(s_w, lane, M, capA[la]);
#pragma unroll
    for (int lb = 0; lb < NB; lb++) {
      const V3 r = A.p - B[lb].p;
      float s, t;
      px_seg_seg(r, A.d, B[lb].d, s, t);
      const V3 cb = B[lb].p + t * B[lb].d;
      const V3 df = (A.p + s * A.d) - cb;
      const float l = sqrtf(dot(df, df));
      const bool far = l >= 1e-9f;
      const float il = 1.f / (far ? l : 1.f);
      const V3 n = px_sel(far, il * df, v3(0, 0, 1));
      const float dist = l - A.r - B[lb].r;
      const int idx = pair0 + la * NB + lb;
      if (want_pd) s_w[(PX_PD + idx) * KD_LD + lane] = dist;
      const bool take = (la == 0 && lb == 0) || dist < best;
      best = take ? dist : best;
      bn = px_sel(take, n, bn);
      bp = px_sel(take, cb + B[lb].r * n, bp);
      bi = take ? idx : bi;
    }
  }
  const V3 pw = o5 + bp;
  rec[0] = best; rec[1] = bn.x; rec[2] = bn.y; rec[3] = bn.z;
  rec[4] = pw.x; rec[5] = pw.y; rec[6] = pw.z; rec[7] = __int_as_float(bi);
}

#define PX_NO_RAYS(...) /* nothing rides on the frames of KD_PLACE_HAND here */

__global__ __launch_bounds__(KD_THREADS) void k_proximity(const DevParams* __restrict__ P, ProxArgs K, int N, int NR) {
  __shared__ float s_w[PX_WORDS * KD_LD];
  __shared__ int s_valid[64];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const DexHandModel& M = P->model;

  bool valid;
  KD_PLACE_HAND(valid, PX_CAP, PX_O5, PX_NO_RAYS, PX_NO_RAYS)   // ---- phase A
  __syncthreads();

  // ---- phase B
  const size_t row = (size_t)blockIdx.x * 64 + lane;
  const V3 o5 = v3(s_w[PX_O5 * KD_LD + lane], s_w[(PX_O5 + 1) * KD_LD + lane], s_w[(PX_O5 + 2) * KD_LD + lane]);

  if (K.cap_env) {
    const bool has_box = K.box.pose != nullptr || K.box.env != 0;   // the same for every row of the call
    KD_LOAD_BOX(bc, bq, row, valid, K.box.env)
    const M3 Rb = q2mat(bq);
    const V3 ob = o5 - bc;   // the one difference of world coordinates
    const float inf = __int_as_float(0x7f800000);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = f + 5 * i;
      if (c < DEXSIM_NCAP) {   // wave-uniform
        const PxSeg S = px_load_seg(s_w, lane, M, c);
        float* const out = K.cap_env + (row * DEXSIM_NCAP + c) * 16;
        float bd = inf, bt = 0.f;
        V3 bn = v3(0, 0, 0), bpw = v3(0, 0, 0);
        if (has_box) {
          V3 nl, pl;
          px_capsule_box(mulT(Rb, ob + S.p), mulT(Rb, S.d), S.r, K.box.hb, nl, pl, bd, bt);
          bn = mul(Rb, nl);
          bpw = mul(Rb, pl) + bc;
        }
        // ground plane z = 0: the lower end of the axis (a tie: t = 0)
        const V3 e0 = o5 + S.p, e1 = e0 + S.d;
        const bool up = e1.z < e0.z;
        const V3 el = px_sel(up, e1, e0);
        if (valid) {
          st4_global(out, bd, bn.x, bn.y, bn.z);
          st4_global(out + 4, bpw.x, bpw.y, bpw.z, bt);
          st4_global(out + 8, el.z - S.r, 0.f, 0.f, 1.f);
          st4_global(out + 12, el.x, el.y, 0.f, up ? 1.f : 0.f);
        }
      }
    }
  }

  if (K.self_min || K.pair_dist) {
    const bool want_pd = K.pair_dist != nullptr;
    float rec[8];
#pragma unroll
    for (int gi = 0; gi < 2; gi++) {   // finger groups 2 f, 2 f + 1
      const int g = 2 * f + gi, fa = px_group_fa(g), fb = px_group_fb(g);
      const int capA[3] = {kd_finger_cap(fa, 0), kd_finger_cap(fa, 1), kd_finger_cap(fa, 2)};
      const int capB[3] = {kd_finger_cap(fb, 0), kd_finger_cap(fb, 1), kd_finger_cap(fb, 2)};
      px_group<3>(s_w, lane, M, capA, capB, 9 * g, o5, want_pd, rec);
      if (K.self_min && valid) {
        float* const out = K.self_min + (row * DEXSIM_NPROX_GROUPS + g) * 8;
        st4_global(out, rec[0], rec[1], rec[2], rec[3]);
        st4_global(out + 4, rec[4], rec[5], rec[6], rec[7]);
      }
    }
    {   // palm group 10 + f: the palm capsules against the middle and distal link of finger f
      const int capA[3] = {0, 1, 2};
      const int capB[3] = {kd_finger_cap(f, 1), kd_finger_cap(f, 2), 0};
      px_group<2>(s_w, lane, M, capA, capB, 90 + 6 * f, o5, want_pd, rec);
      if (K.self_min && valid) {
        float* const out = K.self_min + (row * DEXSIM_NPROX_GROUPS + 10 + f) * 8;
        st4_global(out, rec[0], rec[1], rec[2], rec[3]);
        st4_global(out + 4, rec[4], rec[5], rec[6], rec[7]);
      }
    }
  }

  if (K.pair_dist) {   // ---- phase C
    __syncthreads();   // K.pair_dist is the same for every thread of the launch
    kd_flush<true>(s_w, s_valid, PX_PD, DEXSIM_NPROX_PAIRS, K.pair_dist);
  }
}
