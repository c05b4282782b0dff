// dexsim_raycast.hip.inc -- range sensors of the hand (dexsim_raycast): a few dozen arbitrary rays, each mounted on a joint frame of
// the hand or on the env's world frame, cast against everything the engine collides -- DEXSIM_NCAP capsules, the cube, the ground
// plane -- by the intersection rule of the camera sensors (dexsim_render.hip.inc; the contract is in include/dexsim_ray.h).  A pure
// function of q and the box pose, like the camera and the clearances: one kernel, no workspace, not on the step path; it reads q
// (arena rows or the caller's override) and the box pose (arena rows or the caller's) and writes caller-owned memory only.
// k_render_rays cannot serve: all rays of an image share one eye, so its per-capsule constants live in the scene record, and it has
// no notion of a ray that rides on a joint frame.
//
// One workgroup in the shape of dexsim_chain.hip.inc (64 rows x 5 waves, [word][row] LDS, o5-relative positions); blockIdx.y is the
// chunk of RC_CHUNK rays.  Every workgroup repeats the walk and the chunk index says what it keeps of it, as in k_kin_fk.
//   phase A  the scene stage of dexsim_chain.hip.inc (KD_PLACE_HAND): the axis ends of the capsules relative to o5, and o5 (world),
//            in LDS.  While a wave stands on frame j (the stage's ON_FRAME) it turns the rays of the chunk that ride on j into
//            o5-relative origin and unit direction (rc_put_rays): its range of the sorted list is wave-uniform, from the prefix
//            offsets the entry point hands over (the jstart of FwdKin), so no wave scans a list at a frame.  Wave 0 also takes the
//            world rays.  The ray table is wave-uniform and read through a const __restrict__ pointer at uniform indices: scalar
//            loads.
//   phase B  after one __syncthreads() the lanes stay on their rows and wave w takes the rays w, w + 5, ... of the chunk: ground,
//            box and the 18 capsules, fully unrolled -- independent chains with one strict-less minimum between them.  The loop
//            over a wave's rays is NOT unrolled: every ray runs the same instructions wherever it stands in a call, so a ray of a
//            long list gives the bits of the same ray cast alone.  The hit record overwrites the ray's own eight LDS words (the same
//            thread read them).
//   phase C  after a second __syncthreads() the records leave through kd_flush as contiguous 16-byte stores, the distances (word 0
//            of every record) as contiguous words.
// Plain __syncthreads() only: no atomics, no spins.  A row >= k or with an id outside [0, num_envs) never writes caller memory.
//
// Numerics: every difference is formed between o5-relative numbers of hand size; the box (KD_LOAD_BOX) enters through (o5 - centre)
// rotated into box coordinates once per row, the ground through the world height of the origin, and the world position of o5 is
// added once, to the hit point.  Cylinder: h = r^2 A - (d . (u x o))^2 as in k_render_rays; the end spheres the same way,
// h = r^2 - |d x o'|^2.
//
// Chunk size: 16 rays x 8 words + 111 words of capsules and o5 are 239 words x 65 rows x 4 bytes = 62 140 bytes of LDS.  Eight words
// per ray (six would hold the ray) so that a record is staged in place; see profiles/ray_sensors/README.md for the alternatives.

#define RC_CHUNK 16                            /* rays per workgroup (grid y) */
#define RC_CAP 0                               /* [DEXSIM_NCAP][6] axis ends p0.xyz p1.xyz relative to o5 */
#define RC_O5 (6 * DEXSIM_NCAP)                /* [3] o5, world */
#define RC_RAY (RC_O5 + 3)                     /* [RC_CHUNK][8] origin relative to o5 and unit direction, then the ray's hit record */
#define RC_WORDS (RC_RAY + 8 * RC_CHUNK)
static_assert(RC_WORDS * KD_LD * 4 + 512 <= 65536, "k_raycast: static LDS above 64 KiB");
static_assert(DEXSIM_RAY_MAX <= 65535, "the prefix offsets of the parent groups are 16-bit");

struct RayArgs {
  KinRows rows;
  KinBox box;
  const float* rays;       // (nrays, 6) origin and direction in the parent frame, sorted by parent
  int nrays;
  float tmin, tmax;        // the range window on t
  float* dist;             // (k, nrays) or NULL
  float* hits;             // (k, nrays, 8) or NULL
  // rays [jstart[j + 1], jstart[j + 2]) ride on joint frame j (j = -1: the env's world frame)
  unsigned short jstart[DEXSIM_NJ + 2];
  // DEXSIM_RAY_SKIP_PARENT: bit c of skip[j] is set when capsule c rides on joint frame j (model.cap_parent[c] == j); else zeros
  unsigned skip[DEXSIM_NJ];
};

// The rays of the chunk [r0, r0 + nc) that ride on frame j (origin o relative to o5, orientation qf; WORLD: j = -1, the env's world
// frame, o = -o5, qf is not used): origin and unit direction relative to o5 into the ray's slot, its parent and whether it can hit
// into s_par.
template <bool WORLD>
DI void rc_put_rays(const RayArgs& K, const float* __restrict__ rays, float* s_w, int* s_par, int lane, int r0, int nc, int j, V3 o, Q4 qf) {
  const int lo = max((int)K.jstart[j + 1], r0), hi = min((int)K.jstart[j + 2], r0 + nc);
  if (lo >= hi) return;   // wave-uniform
  const M3 R = q2mat(qf);
  for (int i = lo; i < hi; i++) {
    const float* __restrict__ const r = rays + 6 * (size_t)i;
    const V3 pl = v3(r[0], r[1], r[2]), dl = v3(r[3], r[4], r[5]);
    const float n2 = dot(dl, dl);
    const bool live = n2 >= 1e-24f && n2 < __builtin_inff();
    const float in = 1.f / sqrtf(live ? n2 : 1.f);
    const V3 du = in * dl;
    const V3 p = WORLD ? pl + o : o + mul(R, pl);
    const V3 d = WORLD ? du : mul(R, du);
    const int w = RC_RAY + 8 * (i - r0);
    KD_PUT3(w, p); KD_PUT3(w + 3, d);
    s_par[i - r0] = live ? j : -2;   // every lane the same value
  }
}

// what k_raycast runs on the frames of KD_PLACE_HAND, in its scope
#define RC_WORLD_RAYS(o) rc_put_rays<true>(K, rays, s_w, s_par, lane, r0, nc, -1, o, Q4{0.f, 0.f, 0.f, 1.f})
#define RC_FRAME_RAYS(j, o, q) rc_put_rays<false>(K, rays, s_w, s_par, lane, r0, nc, j, o, q)

__global__ __launch_bounds__(KD_THREADS) void k_raycast(const DevParams* __restrict__ P, RayArgs K, int N, int NR) {
  __shared__ float s_w[RC_WORDS * KD_LD];
  __shared__ int s_valid[64];
  __shared__ int s_par[RC_CHUNK];
  const int lane = threadIdx.x & 63, f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const Arena& A = P->arena;
  const DexHandModel& M = P->model;
  const float* __restrict__ const rays = K.rays;
  const int r0 = blockIdx.y * RC_CHUNK, nc = min(RC_CHUNK, K.nrays - r0);

  bool valid;
  // ---- phase A: the rays of frame j in front of the capsule that rides on it
  KD_PLACE_HAND(valid, RC_CAP, RC_O5, RC_WORLD_RAYS, RC_FRAME_RAYS)
  __syncthreads();

  // ---- phase B
  const size_t row = (size_t)blockIdx.x * 64 + lane;
  const V3 o5 = v3(s_w[RC_O5 * KD_LD + lane], s_w[(RC_O5 + 1) * KD_LD + lane], s_w[(RC_O5 + 2) * KD_LD + lane]);
  const bool has_box = K.box.pose != nullptr || K.box.env != 0;   // the same for every row of the call
  M3 Rb = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  V3 ob = v3(0, 0, 0);   // o5 - centre in box coordinates
  if (has_box) {
    KD_LOAD_BOX(bc, bq, row, valid, true)
    Rb = q2mat(bq);
    ob = mulT(Rb, o5 - bc);   // the one difference of world coordinates
  }
  const float inf = __builtin_inff();

#pragma unroll 1
  for (int s = f; s < nc; s += DEXSIM_NFINGER) {
    float* const w = s_w + (RC_RAY + 8 * s) * KD_LD + lane;
    const V3 ro = v3(w[0], w[KD_LD], w[2 * KD_LD]), d = v3(w[3 * KD_LD], w[4 * KD_LD], w[5 * KD_LD]);
    const int pj = __builtin_amdgcn_readfirstlane(s_par[s]);   // the ray's parent frame, -2: a ray that never hits
    const float tmax = pj == -2 ? -1.f : K.tmax;               // an empty window
    const unsigned skip = K.skip[max(pj, 0)];                  // wave-uniform; the world frame carries no capsule
    float best = inf;
    int id = DEXSIM_SEG_NONE;
    V3 bn = v3(0, 0, 0);   // the normal of the best hit, of a capsule's times its radius

    {   // ground plane z = 0, two-sided, normal +z
      const float dz = fabsf(d.z) > 1e-30f ? d.z : 1e-30f;
      const float t = -(o5.z + ro.z) / dz;
      const bool take = t >= K.tmin && t <= tmax;
      best = take ? t : best;
      id = take ? DEXSIM_SEG_GROUND : id;
      bn.z = take ? 1.f : 0.f;
    }

    if (has_box) {   // the cube: slabs in box coordinates, the entering hit
      const V3 be = ob + mulT(Rb, ro), dbv = mulT(Rb, d);
      const float bev[3] = {be.x, be.y, be.z}, db[3] = {dbv.x, dbv.y, dbv.z};
      float tn = -inf, tf = inf, sg = 0.f;
      int ax = 0;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float di = fabsf(db[i]) > 1e-30f ? db[i] : 1e-30f;
        const float m = 1.f / di;
        const float t1 = -bev[i] * m - fabsf(m) * K.box.hb, t2 = -bev[i] * m + fabsf(m) * K.box.hb;
        const bool later = t1 > tn;
        tn = later ? t1 : tn;
        ax = later ? i : ax;
        sg = later ? (di > 0.f ? -1.f : 1.f) : sg;   // the entering face: its normal is against the ray
        tf = fminf(tf, t2);
      }
      const bool take = tn <= tf && tn >= K.tmin && tn <= tmax && tn < best;
      const V3 n = mul(Rb, v3(ax == 0 ? sg : 0.f, ax == 1 ? sg : 0.f, ax == 2 ? sg : 0.f));
      best = take ? tn : best;
      id = take ? DEXSIM_SEG_BOX : id;
      bn.x = take ? n.x : bn.x; bn.y = take ? n.y : bn.y; bn.z = take ? n.z : bn.z;   // per component: see px_sel
    }

#pragma unroll
    for (int c = 0; c < DEXSIM_NCAP; c++) {
      const float* const cw = s_w + (RC_CAP + 6 * c) * KD_LD + lane;
      const V3 a = v3(cw[0], cw[KD_LD], cw[2 * KD_LD]), b = v3(cw[3 * KD_LD], cw[4 * KD_LD], cw[5 * KD_LD]);
      const float r = M.cap_r[c], r2 = r * r;
      const V3 ba = b - a;
      const float len = norm(ba);
      const bool isseg = len > 1e-9f;
      const float il = 1.f / (isseg ? len : 1.f);
      const V3 u = v3(isseg ? il * ba.x : 1.f, isseg ? il * ba.y : 0.f, isseg ? il * ba.z : 0.f);
      const float L = isseg ? len : 0.f;
      const V3 o = ro - a, o1 = ro - b;
      const float ud = dot(u, d), uo = dot(u, o), od = dot(o, d), od1 = dot(o1, d);
      float t = inf, y = 0.f;
      {   // cylinder body
        const float nd = dot(d, cross(u, o));
        const float Aq = 1.f - ud * ud, Bq = od - uo * ud, h = r2 * Aq - nd * nd;
        const bool ok = h >= 0.f && Aq > 1e-12f;
        const float tb = (-Bq - sqrtf(ok ? h : 0.f)) / (ok ? Aq : 1.f), yb = uo + tb * ud;
        const bool in = ok && yb > 0.f && yb < L;
        t = in ? tb : t; y = in ? yb : y;
      }
      {   // end sphere at a
        const V3 x = cross(d, o);
        const float h = r2 - dot(x, x);
        const float ts = -od - sqrtf(fmaxf(h, 0.f));
        const bool in = h >= 0.f && ts < t;
        t = in ? ts : t; y = in ? 0.f : y;
      }
      {   // end sphere at b
        const V3 x = cross(d, o1);
        const float h = r2 - dot(x, x);
        const float ts = -od1 - sqrtf(fmaxf(h, 0.f));
        const bool in = h >= 0.f && ts < t;
        t = in ? ts : t; y = in ? L : y;
      }
      const bool take = ((skip >> c) & 1u) == 0 && t >= K.tmin && t <= tmax && t < best;
      const V3 n = (o + t * d) - y * u;   // r times the unit normal
      best = take ? t : best;
      id = take ? DEXSIM_SEG_CAPSULE0 + c : id;
      bn.x = take ? n.x : bn.x; bn.y = take ? n.y : bn.y; bn.z = take ? n.z : bn.z;
    }

    const bool hit = id != DEXSIM_SEG_NONE;
    if (id >= DEXSIM_SEG_CAPSULE0) bn = (1.f / norm(bn)) * bn;
    const V3 p = o5 + (ro + best * d);
    w[0] = best;
    w[KD_LD] = hit ? p.x : 0.f; w[2 * KD_LD] = hit ? p.y : 0.f; w[3 * KD_LD] = hit ? p.z : 0.f;
    w[4 * KD_LD] = hit ? bn.x : 0.f; w[5 * KD_LD] = hit ? bn.y : 0.f; w[6 * KD_LD] = hit ? bn.z : 0.f;
    w[7 * KD_LD] = __int_as_float(id);
  }
  __syncthreads();

  // ---- phase C
  if (K.hits) kd_flush<true>(s_w, s_valid, RC_RAY, 8 * nc, K.hits, 8 * (size_t)K.nrays, 8 * (size_t)r0);
  if (K.dist) {   // word 0 of every record, along the contiguous output index
    const size_t row0 = (size_t)blockIdx.x * 64;
    for (int idx = threadIdx.x; idx < 64 * nc; idx += KD_THREADS) {
      const int r = idx / nc, c = idx - r * nc;
      if (s_valid[r]) GPTR(K.dist)[(row0 + r) * K.nrays + r0 + c] = s_w[(RC_RAY + 8 * c) * KD_LD + r];
    }
  }
}
