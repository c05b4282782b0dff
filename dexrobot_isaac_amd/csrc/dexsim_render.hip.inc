// dexsim_render.hip.inc -- camera sensors (dexsim_render): depth, segmentation and colour images by exact ray casting.
//
// Everything the engine collides is analytic (18 capsules, one cube, the ground plane), so an image is ~20 closed-form ray tests per
// pixel.  Two kernels, neither on the step path; both read persistent state only and write caller-owned memory only:
//
//   k_render_scene  one lane per rendered env (64 envs per wave, q rows read coalesced like publish_body): walks the chain from q
//                   in world coordinates -- spawn frame, 6 base joints, 5 x 4 finger joints through joint_frame
//                   (dexsim_chain.hip.inc); never jframe, which is sub-step scratch holding pre-integration frames -- places the capsules and the box, resolves the camera and writes the env's SCENE
//                   RECORD (include/dexsim.h), including everything that is the same for all rays of the image: all rays share
//                   the eye, so o = eye - a, u x o, |o|^2 - r^2 ... are per capsule, not per ray.
//   k_render_rays   grid (ceil(W H / 256), k), 256 threads = 4 waves, one lane per pixel, row-major.  All lanes of a wave belong
//                   to one image, so the scene record is wave-uniform: it is read through a const __restrict__ pointer indexed by
//                   blockIdx.y and compile-time offsets only, i.e. with s_load_dwordx* through the scalar cache into SGPRs -- no
//                   per-lane copy of the record exists.  No LDS, no barriers, no atomics, no spins.  Nearest hit with its id and
//                   its diffuse term, then up to three fully coalesced stores per wave (depth, seg, rgba as one packed word).
//
// Capsule test (unit axis u, length L, radius r, o = eye - a, ray direction d, |d| = 1): the capsule is the union of the open
// cylinder body and the two end spheres; the first hit of a union of convex bodies is the earliest of their entering hits, and the
// flat ends of the cylinder lie inside the spheres.  Body: A = 1 - (u.d)^2, B = d.o - (u.o)(u.d), discriminant
// h = r^2 A - (d.(u x o))^2 -- this form has no cancellation beyond the silhouette's own --, t = (-B - sqrt(h)) / A, accepted when
// 0 < u.o + t u.d < L.  Spheres: t = -d.o' - sqrt((d.o')^2 - (|o'|^2 - r^2)), o' = o or o - L u.
// Only n.l is needed of the normal: n = (o + t d - y u) / r with y the axis coordinate of the hit (0 / L for the spheres), so
// n.l = (l.o + t l.d - y l.u) / r from two more per-capsule constants.

#define RS_CAM_EYE 0
#define RS_CAM_RIGHT 3
#define RS_CAM_UP 6
#define RS_CAM_FWD 9
#define RS_BOX_CENTER 12
#define RS_BOX_ROT 15
#define RS_BOX_HALF 24
#define RS_BOX_EYE 25
#define RS_BOX_LIGHT 28
#define RS_CAP_RGB 31
#define RS_RESERVED (RS_CAP_RGB + DEXSIM_NCAP)
#define RS_CAPS 52
static_assert(RS_RESERVED <= RS_CAPS && RS_CAPS % 4 == 0 && DEXSIM_RCAP_WORDS % 4 == 0, "capsule blocks are written as 16-byte quads");
static_assert(DEXSIM_SCENE_WORDS == RS_CAPS + DEXSIM_NCAP * DEXSIM_RCAP_WORDS && DEXSIM_SCENE_WORDS % 4 == 0, "scene record layout");

struct RenderSection { const char* name; int words, is_int, off; };
static const RenderSection kRenderSections[] = {
    {"cam_eye", 3, 0, RS_CAM_EYE}, {"cam_right", 3, 0, RS_CAM_RIGHT}, {"cam_up", 3, 0, RS_CAM_UP}, {"cam_forward", 3, 0, RS_CAM_FWD},
    {"box_center", 3, 0, RS_BOX_CENTER}, {"box_rot", 9, 0, RS_BOX_ROT}, {"box_half", 1, 0, RS_BOX_HALF},
    {"box_eye", 3, 0, RS_BOX_EYE}, {"box_light", 3, 0, RS_BOX_LIGHT}, {"cap_rgb", DEXSIM_NCAP, 1, RS_CAP_RGB},
    {"reserved", RS_CAPS - RS_RESERVED, 0, RS_RESERVED}, {"capsules", DEXSIM_NCAP * DEXSIM_RCAP_WORDS, 0, RS_CAPS}};

DI unsigned render_rgb(int p) {   // palette entry p packed R | G << 8 | B << 16
  constexpr unsigned char pal[DEXSIM_RENDER_NPALETTE][3] = DEXSIM_RENDER_PALETTE;
  return (unsigned)pal[p][0] | (unsigned)pal[p][1] << 8 | (unsigned)pal[p][2] << 16;
}
#define RENDER_RGB(p) render_rgb(p)

struct RenderArgs {
  DexSimCamera cam;
  const float* eye;         // (k, 3) per-env overrides or NULL
  const float* target;
  const int64_t* env_ids;   // k ids or NULL = identity
  int k, img0;              // images of the call; first image of this launch (the grid's y extent is limited)
  float tan_x, tan_y;       // tan(hfov / 2) and the same times H / W
};

DI V3 normalized(V3 v) { const float s = 1.f / norm(v); return s * v; }

// -------------------------------------------------------------------------------------------------- scene records
// MOUNTED: the camera rides on a joint frame (parent_joint >= 0); the world camera does not track a parent frame.
template <bool MOUNTED>
__global__ __launch_bounds__(64) void k_render_scene(const DevParams* __restrict__ P, RenderArgs R, float* __restrict__ scene, int N, int NR) {
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (l >= R.k) return;
  const long long id = R.env_ids ? R.env_ids[l] : (long long)l;
  if (id < 0 || id >= NR) return;   // renders nothing
  const int e = (int)id;
  const Arena& A = P->arena;
  const DexHandModel& M = P->model;
  const DexSimConfig& C = P->cfg;
  float* const S = scene + (size_t)l * DEXSIM_SCENE_WORDS;
  const float light[3] = DEXSIM_RENDER_LIGHT;
  const V3 lw = v3p(light);

  // parent frame of the camera: the world, or the joint frame picked up during the walk
  V3 po = {0, 0, 0};
  M3 pR = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  const int pj = MOUNTED ? R.cam.parent_joint : -1;

  // capsule endpoints are collected first (the camera may ride on a later joint than a capsule's), the records follow.
  // validate_model: capsules 0-2 ride on the palm joint 5, capsule 3 + 3 f + i on joint 6 + 4 f + 1 + i.
  V3 ca[DEXSIM_NCAP], cb[DEXSIM_NCAP];
  auto place_cap = [&](int c, V3 o, const M3& Rj) { ca[c] = o + mul(Rj, v3p(M.cap_p0[c])); cb[c] = o + mul(Rj, v3p(M.cap_p1[c])); };

  Q4 qc = q4p(M.spawn_quat);
  V3 oc = v3p(M.spawn_pos);
#pragma unroll
  for (int j = 0; j < 6; j++) {   // base chain: world origins, (o + d) + q aw like publish_body
    const float qj = FLD(q, j);
    const JointFrame F = joint_frame(P->jc[j], qj, qc, j < 3);
    V3 on = oc + F.d;
    if (j < 3) on += qj * F.aw;
    qc = F.qn; oc = on;
    if (j == pj) { po = oc; pR = q2mat(qc); }
  }
  const Q4 q5 = qc; const V3 o5 = oc;
  {
    const M3 R5 = q2mat(q5);
#pragma unroll
    for (int c = 0; c < 3; c++) place_cap(c, o5, R5);
  }
#pragma unroll
  for (int f = 0; f < DEXSIM_NFINGER; f++) {
    Q4 qf = q5; V3 of = o5;
#pragma unroll
    for (int lk = 0; lk < DEXSIM_NFJ; lk++) {
      const int j = 6 + 4 * f + lk;
      V3 aw;
      kd_finger_joint(P->jc[j], FLD(q, j), of, qf, aw);
      const M3 Rj = q2mat(qf);
      if (j == pj) { po = of; pR = Rj; }
      if (lk >= 1) place_cap(3 + 3 * f + lk - 1, of, Rj);
    }
  }

  // ---- camera: look-at in the parent frame, up = the parent's +z
  V3 le = v3p(R.cam.eye), lt = v3p(R.cam.target);
  if (R.eye) le = v3p(R.eye + 3 * (size_t)l);
  if (R.target) lt = v3p(R.target + 3 * (size_t)l);
  const V3 eye = po + mul(pR, le);
  V3 fl = lt - le;   // view direction in parent coordinates
  const float fn = norm(fl);
  fl = fn > 1e-12f ? (1.f / fn) * fl : v3(1, 0, 0);
  const bool along_z = fl.x * fl.x + fl.y * fl.y < 1e-12f;   // sine of the angle to the parent's z axis below 1e-6
  const V3 upl = along_z ? v3(0, 1, 0) : v3(0, 0, 1);
  const V3 rl = normalized(cross(fl, upl));
  const V3 ul = cross(rl, fl);
  const V3 fwd = mul(pR, fl), right = mul(pR, rl), up = mul(pR, ul);
  S[RS_CAM_EYE] = eye.x; S[RS_CAM_EYE + 1] = eye.y; S[RS_CAM_EYE + 2] = eye.z;
  S[RS_CAM_RIGHT] = right.x; S[RS_CAM_RIGHT + 1] = right.y; S[RS_CAM_RIGHT + 2] = right.z;
  S[RS_CAM_UP] = up.x; S[RS_CAM_UP + 1] = up.y; S[RS_CAM_UP + 2] = up.z;
  S[RS_CAM_FWD] = fwd.x; S[RS_CAM_FWD + 1] = fwd.y; S[RS_CAM_FWD + 2] = fwd.z;

  // ---- box
  {
    M3 Rb = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    V3 bc = {0, 0, 0};
    float half = 0.f;
    if (C.has_box) {
      bc = v3(FLD(box_pos, 0), FLD(box_pos, 1), FLD(box_pos, 2));
      Rb = q2mat(Q4{FLD(box_quat, 0), FLD(box_quat, 1), FLD(box_quat, 2), FLD(box_quat, 3)});
      half = 0.5f * C.box_size;
    }
    const V3 be = mulT(Rb, eye - bc), bl = mulT(Rb, lw);
    S[RS_BOX_CENTER] = bc.x; S[RS_BOX_CENTER + 1] = bc.y; S[RS_BOX_CENTER + 2] = bc.z;
#pragma unroll
    for (int i = 0; i < 9; i++) S[RS_BOX_ROT + i] = Rb.m[i];
    S[RS_BOX_HALF] = half;
    S[RS_BOX_EYE] = be.x; S[RS_BOX_EYE + 1] = be.y; S[RS_BOX_EYE + 2] = be.z;
    S[RS_BOX_LIGHT] = bl.x; S[RS_BOX_LIGHT + 1] = bl.y; S[RS_BOX_LIGHT + 2] = bl.z;
  }
#pragma unroll
  for (int i = RS_RESERVED; i < RS_CAPS; i++) S[i] = 0.f;

  // ---- capsules
#pragma unroll
  for (int c = 0; c < DEXSIM_NCAP; c++) {
    const int fs = M.cap_fslot[c];
    const int pal = fs == DEXSIM_FSLOT_PALM ? 2 : 3 + min(fs / 3, DEXSIM_NFINGER - 1);
    ((unsigned*)S)[RS_CAP_RGB + c] = RENDER_RGB(pal);
    const V3 a = ca[c], b = cb[c];
    const float r = M.cap_r[c];
    const V3 ba = b - a;
    const float len = norm(ba);
    const V3 u = len > 1e-9f ? (1.f / len) * ba : v3(1, 0, 0);
    const V3 o = eye - a, ob = eye - b;
    const V3 n = cross(u, o);
    float* const D = S + RS_CAPS + c * DEXSIM_RCAP_WORDS;
    st4_global(D + DEXSIM_RCAP_A, a.x, a.y, a.z, r);
    st4_global(D + DEXSIM_RCAP_B, b.x, b.y, b.z, len > 1e-9f ? len : 0.f);
    st4_global(D + DEXSIM_RCAP_U, u.x, u.y, u.z, dot(u, o));
    st4_global(D + DEXSIM_RCAP_O, o.x, o.y, o.z, 1.f / r);
    st4_global(D + DEXSIM_RCAP_N, n.x, n.y, n.z, dot(o, o) - r * r);
    st4_global(D + DEXSIM_RCAP_CB, dot(ob, ob) - r * r, dot(lw, o), dot(lw, u), r * r);
  }
}

// -------------------------------------------------------------------------------------------------- rays
struct RayOut { float* depth; unsigned* rgba; int* seg; };

// HAS_BOX: the configuration has a box (DexSimConfig::has_box; the record's box_half is then positive).
template <bool HAS_BOX>
__global__ __launch_bounds__(256) void k_render_rays(const float* __restrict__ scene, RenderArgs R, RayOut O, int NR) {
  const int img = R.img0 + blockIdx.y;   // wave-uniform: everything read from the record below is a scalar load
  if (R.env_ids) {
    const long long id = R.env_ids[img];
    if (id < 0 || id >= NR) return;      // renders nothing
  }
  const float* __restrict__ const S = scene + (size_t)img * DEXSIM_SCENE_WORDS;
  const int W = R.cam.width, npix = W * R.cam.height;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool live = p < npix;            // the last wave of an image is partial whenever W H is not a multiple of 64
  const int pc = live ? p : npix - 1;
  const int py = pc / W, px = pc - py * W;
  const float sx = (2.f * ((float)px + 0.5f) / (float)W - 1.f) * R.tan_x;
  const float sy = (1.f - 2.f * ((float)py + 0.5f) / (float)R.cam.height) * R.tan_y;
  V3 d = v3p(S + RS_CAM_FWD) + sx * v3p(S + RS_CAM_RIGHT) + sy * v3p(S + RS_CAM_UP);
  const float cosax = 1.f / norm(d);     // d . forward after normalisation: depth = t * cosax
  d = cosax * d;
  const float light[3] = DEXSIM_RENDER_LIGHT;
  const float ld = light[0] * d.x + light[1] * d.y + light[2] * d.z;
  // depth window as a window on t
  const float tmin = fmaxf(R.cam.near_clip, 0.f) / cosax, tmax = R.cam.far_clip / cosax;

  float best = __builtin_inff(), ndl = 0.f;
  int id = DEXSIM_SEG_NONE;
  unsigned rgb = 0;
  auto take = [&](float t, float n_dot_l, int seg_id, unsigned colour) {
    if (t >= tmin && t <= tmax && t < best) { best = t; ndl = n_dot_l; id = seg_id; rgb = colour; }
  };

  {   // ground plane z = 0, normal +z
    const float ez = S[RS_CAM_EYE + 2];
    const float dz = fabsf(d.z) > 1e-30f ? d.z : 1e-30f;
    take(-ez / dz, light[2], DEXSIM_SEG_GROUND, RENDER_RGB(0));
  }

  if (HAS_BOX) {   // oriented box: slabs in box coordinates
    const float hb = S[RS_BOX_HALF];
    const float* Rb = S + RS_BOX_ROT;
    const float db[3] = {Rb[0] * d.x + Rb[3] * d.y + Rb[6] * d.z, Rb[1] * d.x + Rb[4] * d.y + Rb[7] * d.z,
                         Rb[2] * d.x + Rb[5] * d.y + Rb[8] * d.z};
    float tn = -__builtin_inff(), tf = __builtin_inff(), nl = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const float di = fabsf(db[i]) > 1e-30f ? db[i] : 1e-30f;
      const float m = 1.f / di;
      const float t1 = -S[RS_BOX_EYE + i] * m - fabsf(m) * hb, t2 = -S[RS_BOX_EYE + i] * m + fabsf(m) * hb;
      if (t1 > tn) { tn = t1; nl = di > 0.f ? -S[RS_BOX_LIGHT + i] : S[RS_BOX_LIGHT + i]; }   // entering face: normal against the ray
      tf = fminf(tf, t2);
    }
    if (tn <= tf) take(tn, nl, DEXSIM_SEG_BOX, RENDER_RGB(1));
  }

#pragma unroll
  for (int c = 0; c < DEXSIM_NCAP; c++) {
    const float* D = S + RS_CAPS + c * DEXSIM_RCAP_WORDS;
    const float L = D[DEXSIM_RCAP_LEN], uo = D[DEXSIM_RCAP_UO], r2 = D[DEXSIM_RCAP_R2];
    const float ud = D[DEXSIM_RCAP_U] * d.x + D[DEXSIM_RCAP_U + 1] * d.y + D[DEXSIM_RCAP_U + 2] * d.z;
    const float od = D[DEXSIM_RCAP_O] * d.x + D[DEXSIM_RCAP_O + 1] * d.y + D[DEXSIM_RCAP_O + 2] * d.z;
    const float nd = D[DEXSIM_RCAP_N] * d.x + D[DEXSIM_RCAP_N + 1] * d.y + D[DEXSIM_RCAP_N + 2] * d.z;
    float t = __builtin_inff(), y = 0.f;
    {   // cylinder body
      const float Aq = 1.f - ud * ud, Bq = od - uo * ud, h = r2 * Aq - nd * nd;
      if (h >= 0.f && Aq > 1e-12f) {
        const float tb = (-Bq - sqrtf(h)) / Aq, yb = uo + tb * ud;
        if (yb > 0.f && yb < L) { t = tb; y = yb; }
      }
    }
    {   // end sphere at a
      const float h = od * od - D[DEXSIM_RCAP_CA];
      if (h >= 0.f) { const float ts = -od - sqrtf(h); if (ts < t) { t = ts; y = 0.f; } }
    }
    {   // end sphere at b: o' = o - L u
      const float odb = od - L * ud, h = odb * odb - D[DEXSIM_RCAP_CB];
      if (h >= 0.f) { const float ts = -odb - sqrtf(h); if (ts < t) { t = ts; y = L; } }
    }
    const float nl = (D[DEXSIM_RCAP_LO] + t * ld - y * D[DEXSIM_RCAP_LU]) * D[DEXSIM_RCAP_INVR];
    take(t, nl, DEXSIM_SEG_CAPSULE0 + c, ((const unsigned*)S)[RS_CAP_RGB + c]);
  }

  if (!live) return;   // never a store outside k H W
  const size_t o = (size_t)img * (size_t)npix + (size_t)p;
  const bool hit = id != DEXSIM_SEG_NONE;
  if (O.depth) GPTR(O.depth)[o] = hit ? best * cosax : __builtin_inff();
  if (O.seg) GPTR(O.seg)[o] = id;
  if (O.rgba) {
    const unsigned char bg[3] = DEXSIM_RENDER_BACKGROUND;
    unsigned w = 0xff000000u | (unsigned)bg[0] | (unsigned)bg[1] << 8 | (unsigned)bg[2] << 16;
    if (hit) {
      const float shade = DEXSIM_RENDER_AMBIENT + (1.f - DEXSIM_RENDER_AMBIENT) * fminf(fmaxf(ndl, 0.f), 1.f);
      const unsigned r = (unsigned)((float)(rgb & 255u) * shade + 0.5f), g = (unsigned)((float)((rgb >> 8) & 255u) * shade + 0.5f),
                     b = (unsigned)((float)((rgb >> 16) & 255u) * shade + 0.5f);
      w = 0xff000000u | r | g << 8 | b << 16;
    }
    GPTR(O.rgba)[o] = w;
  }
}
